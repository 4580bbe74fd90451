"""The plants of the cell grid (tests/planted_samples.py, its third part) shown decisive on the restatements alone, no GPU:
what tests/test_gpu_planted_cells.py feeds to the kernels of draw_focus.hip and draw_aim.hip does sit on the decision it is
named after, and replacing a plant by its neighbour changes what the restatement computes.

  A. the cell-list source (six draws per sample; tests/focus_reference.c, tests/aim_reference.c, tests/cells_reference.h)
     0. plant_outputs plants any six outputs, and the restatements' mapping equals the Fraction reference on every sextuple;
     1. the entry draw either side of a boundary of j selects cells far apart;
     2. offset draws 0 and 2^53 - 1: the next cell's corner, and 2 exactly in the last column and row;
     3. corner + offset on a tie: the reference moves by one ulp across it and the two-rounding sum disagrees;
     4. one ulp below a marked cell of the interior map c_re + 2 rounds onto the marked column, the exact column does not;
     5. adjacent doubles off the 2^-51 grid that the cardioid's and the bulb's test tell apart.
  B. the mask sink (four draws per sample)
     1. a sample on a cell's edge and its grid neighbour below set different bits: bit 0 and 31, the first and last word;
     2. under a fixed c the bit is z_0's;
     3. the replay ends at the first point on the canvas: replay_steps is its index;
     4. samples that are too fast, never escape or are rejected mark nothing;
     5. the bounded kind: the first point on the canvas in the transient, in the period, nowhere.

A sample of the cell source is read off the histogram of the aimed draw on --plane cr,ci, where every plotted point is c
itself, on a canvas whose pixels are ONE ULP wide (planted_samples.ulp_canvas): the planted sample is alone in the centre
pixel, its neighbour in the pixel beside it.  Every comparison is bit for bit; no tolerance appears anywhere."""

import math
from fractions import Fraction

import numpy as np
import pytest

import aim_reference as aim
import focus_reference as focus
import planted_samples as P
import plot_reference as plot

W, H = 64, 48
CENTRE = (H // 2, W // 2)


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return aim.load(tmp_path_factory.mktemp("aim_ref"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return plot.load(tmp_path_factory.mktemp("plot_ref"))


def aim_draw(aref, level, cells, draws, box, launches=(1,), max_iter=P.CELL_MAX_ITER):
    """The aimed draw of --plane cr,ci from the planted states -> (hist, counters)."""
    return aim.draw(aref, cells, states=P.plant_cell_states(draws), w=W, h=H, box=box, max_iter=max_iter, min_iter=0,
                    threads=len(draws), level=level, draw=tuple(launches), projection=P.C_PLANE)


def focus_draw(aref, level, cells, draws, box=P.WIDE_BOX, launches=(1,)):
    return focus.draw(aref.focus, W, H, P.CELL_MAX_ITER, 0, len(draws), list(launches), box=box, level=level,
                      cell_list=cells, states=P.plant_cell_states(draws))


def alone_in(hist, pixel):
    return hist[pixel] > 0 and int(hist.sum()) == int(hist[pixel])


def mapped(aref, level, cells, draws):
    """The two restatements' mapping of the draws, asserted equal -> (j, re, im)."""
    o = P.cell_outputs(*draws, low=0x5A5)
    got = focus.mapping(aref.focus, level, cells, *o)
    assert got == aim.mapping(aref, level, cells, *o)
    return got


# ---- A0. the planting, and the mapping against the Fraction reference ------------------------------------------------------


def test_plant_outputs_plants_any_six_outputs():
    top = 0xFFFFFFFF
    rng = np.random.default_rng(6)
    targets = [(0,) * 6, (top,) * 6, (0, top, 0, top, 0, top), (top, 0, top, 0, top, 0)]
    targets += [tuple(int(v) for v in rng.integers(0, 1 << 32, 6)) for _ in range(12)]
    for o in targets:
        for start in (0, 0x9E3779B9):
            got = P.six_outputs(P.plant_outputs(o, start=start))
            assert got[:5] == list(o[:5]) and got[5] >> 11 == o[5] >> 11, (o, got)
    # fewer free bits: rarer, still exact; and two starts give two states with two continuations
    got = P.six_outputs(P.plant_outputs(targets[5], free_low_bits_of_o6=8))
    assert got[:5] == list(targets[5][:5]) and got[5] >> 8 == targets[5][5] >> 8
    a, b = P.plant_outputs(targets[4], start=1), P.plant_outputs(targets[4], start=1 << 31)
    assert int(a["d"]) != int(b["d"])


def every_sextuple():
    """(level, list, draws) of every cell case."""
    out = []
    for name in P.LIST_SIZES:
        level, cells, plants = P.entry_plants(name)
        out += [(level, cells, d) for d, _ in plants]
    for level in (4, 10):
        for _, cells, d, neighbour in P.offset_plants(level):
            out += [(level, cells, d)] + ([(level, cells, neighbour)] if neighbour else [])
        for axis in (0, 1):
            out += [(level, cells, d) for _, cells, d, _, _ in P.tie_plants(level, axis)]
    for _, _, cells, below, on, _ in P.map_plants():
        out += [(10, cells, below), (10, cells, on)]
    for _, cells, inside, outside, _, _ in P.shape_plants():
        out += [(10, cells, inside), (10, cells, outside)]
    return out


def test_the_mapping_is_the_fraction_reference_on_every_planted_sextuple(aref):
    """tests/cells_reference.h's doubles against integers and Fractions rounded once; and the planted state's first six
    outputs, mapped, are that sample."""
    cases = every_sextuple()
    assert len(cases) > 150
    for level, cells, draws in cases:
        assert mapped(aref, level, cells, draws) == P.exact_sample(level, cells, *draws), (level, draws)
    for level, cells, draws in cases[::9]:
        o = P.six_outputs(P.plant_cell_states([draws])[0])
        assert focus.mapping(aref.focus, level, cells, *o) == P.exact_sample(level, cells, *draws)


# ---- A1. entry selection ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(P.LIST_SIZES))
def test_the_entry_draw_either_side_of_a_boundary_selects_cells_far_apart(aref, name):
    level, cells, plants = P.entry_plants(name)
    n = len(cells)
    assert n == P.LIST_SIZES[name][1]
    rows, cols = np.divmod(cells.astype(np.int64), 4 << level)
    far = np.maximum(np.abs(np.diff(rows)), np.abs(np.diff(cols)))            # cells between neighbouring entries
    assert n == 1 or far.min() >= (4 << level) // 16, far.min()
    assert {j for _, j in plants} == {0, 1, n - 2, n - 1} & set(range(n))
    for draws, j in plants:
        assert mapped(aref, level, cells, draws)[0] == j
        mine = aim_draw(aref, level, cells, [draws] * 64, P.SQUARE_C)[0], focus_draw(aref, level, cells, [draws] * 64)[0]
        assert mine[0].sum() > 0 and mine[1].sum() > 0                         # the planted entries are cells outside the set
        for other in (j - 1, j + 1):                                           # a list of one has no other entry
            if 0 <= other < n:
                there = ((2 * other + 1) << 64) // (2 * n), P.MID, P.MID
                assert mapped(aref, level, cells, there)[0] == other
                assert not np.array_equal(aim_draw(aref, level, cells, [there] * 64, P.SQUARE_C)[0], mine[0])
                assert not np.array_equal(focus_draw(aref, level, cells, [there] * 64)[0], mine[1])


# ---- A2. offset extremes --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("level", [4, 10])
def test_offset_draws_zero_and_all_ones(aref, level):
    side, seen = 2.0 ** -level, set()
    for name, cells, draws, neighbour in P.offset_plants(level):
        j, re, im = P.exact_sample(level, cells, *draws)
        corner = P.cell_corner(level, int(cells[j]))
        for v, x, c in ((draws[1], re, corner[0]), (draws[2], im, corner[1])):
            if v == P.V_MAX:
                assert x == float(c) + side                                    # the next cell's corner, on the dot
            if v == 0:
                assert Fraction(x) == c + Fraction(1, 1 << (53 + level)) or x == float(c)
        seen.add((re == 2.0, im == 2.0))
        box = P.ulp_canvas(re, im)
        hist, cnt = aim_draw(aref, level, cells, P.cell_lanes(draws), box)
        assert alone_in(hist, CENTRE) and cnt["recorded"] == 64, name          # the fillers are recorded and off the canvas
        if neighbour is not None:
            assert P.exact_point(level, int(cells[j]), *neighbour[1:]) != (re, im)
            other, _ = aim_draw(aref, level, cells, P.cell_lanes(neighbour), box)
            assert other[CENTRE] == 0, name                                    # a pixel away, or (beside zero) off the canvas
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


# ---- A3. the one rounding -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("axis", [0, 1], ids=["re", "im"])
@pytest.mark.parametrize("level", [4, 10])
def test_corner_plus_offset_is_rounded_once(aref, level, axis):
    plants = P.tie_plants(level, axis)
    disagree = dict.fromkeys(P.CORNER_CLASSES, 0)
    for k in range(0, len(plants), 3):
        (name, cells, below, _, _), (_, _, tie, parity, what), (_, _, above, _, _) = plants[k:k + 3]
        cell = int(cells[0])
        x = [P.exact_point(level, cell, *d[1:])[axis] for d in (below, tie, above)]
        if what == "tie":                                                      # one ulp across the tie, the tie to the even side
            assert x[2] == math.nextafter(x[0], math.inf)
            even = [v for v in (x[0], x[2]) if int(Fraction(v) / Fraction(math.ulp(v))) % 2 == 0]
            assert even == [x[1]]
        else:                                                                  # beside zero the sum is exact: three doubles
            assert what == "exact" and x[0] < x[1] < x[2]
            assert all(Fraction(v) == P.cell_corner(level, cell)[axis] + Fraction(d[1 + axis] + 1, 1 << (53 + level))
                       for v, d in zip(x, (below, tie, above)))
        for d in (below, tie, above):
            point = P.exact_point(level, cell, *d[1:])
            disagree[name] += P.two_roundings(level, cell, *d[1:]) != point
            box = P.ulp_canvas(*point)
            hist, _ = aim_draw(aref, level, cells, P.cell_lanes(d), box)
            assert alone_in(hist, CENTRE), (name, what)
        # the neighbour across the tie lands one pixel away on the tie's canvas
        box = P.ulp_canvas(*P.exact_point(level, cell, *tie[1:]))
        hists = [aim_draw(aref, level, cells, P.cell_lanes(d), box)[0] for d in (below, above)]
        assert not np.array_equal(*hists) and sum(h[CENTRE] > 0 for h in hists) <= 1
    assert all(n > 0 for n in disagree.values()), disagree


# ---- A4. the exact map column ---------------------------------------------------------------------------------------------------


def test_one_ulp_below_a_marked_cell_the_rounded_sum_is_on_it(aref):
    """The restatement has no map: both lanes iterate max_iter steps and never escape, and the histogram is empty either
    way.  What tells the two apart on the device is skipped_steps alone."""
    plants = P.map_plants()
    assert len(plants) >= 2
    for e, im, cells, below, on, map_level in plants:
        x = P.exact_sample(10, cells, *below)[1]
        assert x == math.nextafter(e, -math.inf) and P.exact_sample(10, cells, *on)[1:] == (e, im)
        exact, rounded = P.map_columns(x, map_level)
        assert rounded == exact + 1 == P.map_columns(e, map_level)[0] == P.map_columns(e, map_level)[1]
        for draws in (below, on):
            hist, cnt = aim_draw(aref, 10, cells, P.cell_lanes(draws), P.SQUARE_C, max_iter=100)
            assert (cnt["never_escaped"], cnt["rejected"], cnt["recorded"]) == (1, 0, 63) and cnt["iterate_steps"] == 163


# ---- A5. rejection off the grid -------------------------------------------------------------------------------------------------


def test_adjacent_doubles_off_the_grid_across_the_shapes_edges(aref):
    plants = P.shape_plants()
    assert {p[0] for p in plants} == {"cardioid", "bulb"}
    for shape, cells, inside, outside, a, b in plants:
        assert b[0] in (math.nextafter(a[0], math.inf), math.nextafter(a[0], -math.inf)) and a[1] == b[1]
        assert abs(a[0]) < 1.0 and all(math.ldexp(x, 51) != int(math.ldexp(x, 51)) for x in (a[0], b[0]))
        assert P.exact_sample(10, cells, *inside)[1:] == a and P.exact_sample(10, cells, *outside)[1:] == b
        _, ci = aim_draw(aref, 10, cells, P.cell_lanes(inside, shape="all64"), P.SQUARE_C)
        _, co = aim_draw(aref, 10, cells, P.cell_lanes(outside, shape="all64"), P.SQUARE_C)
        assert ci["rejected"] == 64 and co["rejected"] == 0, shape
        _, fi = focus_draw(aref, 10, cells, P.cell_lanes(inside, shape="all64"))
        _, fo = focus_draw(aref, 10, cells, P.cell_lanes(outside, shape="all64"))
        assert fi["rejected"] == 64 and fo["rejected"] == 0, shape


# ---- B. the mask sink -----------------------------------------------------------------------------------------------------------


def probes(aref, points, level, box, max_iter, min_iter, **kw):
    """The probe of one sample per subsequence by both restatements (the focused one where it is defined: the Mandelbrot
    step on a sampled c, escaping orbits), asserted equal -> (mask, counters)."""
    n = len(points)
    mask, cnt = aim.probe(aref, states=P.plant_states(points), w=W, h=H, box=box, max_iter=max_iter, min_iter=min_iter,
                          threads=n, level=level, probe=(1,), **kw)
    if not kw:
        m2, c2 = focus.probe(aref.focus, W, H, max_iter, min_iter, n, [1], level, box, states=P.plant_states(points))
        assert np.array_equal(m2, mask) and c2 == {k: cnt[k] for k in c2}
    return mask, cnt


def only_bits(mask, level, *samples):
    want = np.zeros_like(mask)
    for s in samples:
        word, bit = P.mask_bit(level, *s)
        want[word] |= np.uint32(1 << bit)
    return np.array_equal(mask, want)


@pytest.mark.parametrize("level", [4, 10])
def test_a_sample_on_a_cell_edge_and_its_neighbour_below_set_different_bits(aref, ref, level):
    samples = P.cell_edge_samples(level)
    words = focus.mask_words(level)
    where = {name: P.mask_bit(level, *s) for name, s in samples}
    assert {0, 31} <= {b for _, b in where.values()} and {0, words - 1} <= {w for w, _ in where.values()}
    n = 4 << level
    for name in ("re = 2", "im = 2", "both = 2"):                              # clamped into the last column, row, cell
        col, row = (where[name][0] * 32 + where[name][1]) % n, (where[name][0] * 32 + where[name][1]) // n
        assert (col == n - 1 or "im" in name) and (row == n - 1 or "re" in name)
    for k in range(0, len(samples) - 4, 2):
        assert where[samples[k][0]] != where[samples[k + 1][0]]                # on the edge / below it
    for name, s in samples:
        for shape in P.SHAPES:
            box = P.box_around(P.z_1(ref, s))
            mask, cnt = probes(aref, P.lanes(s, 64, shape), level, box, P.CELL_MAX_ITER, 0)
            # the fillers are accepted (min_iter 0) and replay their one point, (2, 10): off every canvas here but those of
            # the samples next to (2, 2), whose z_1 is next to it -- there they mark their own cell, the last one
            both = P.filler_marks(box) and shape != "all64"
            lanes = 64 if shape == "all64" or both else 1
            assert only_bits(mask, level, s, *([P.FILLER] if both else [])), name
            assert (cnt["recorded"], cnt["replay_steps"], cnt["too_fast"]) == (lanes, 64, 0), (name, cnt)


def test_under_a_fixed_c_the_bit_is_the_cell_of_z_0(aref, ref):
    z0 = P.with_end(ref, 13, P.FIXED_C)
    for level in (6, 10):
        assert P.mask_bit(level, *z0)[0] != P.mask_bit(level, *P.FIXED_C)[0]   # another word
        for shape in P.SHAPES:
            mask, cnt = probes(aref, P.lanes(z0, 64, shape), level, P.WIDE_BOX, 20, 1, c=P.FIXED_C)
            lanes = 64 if shape == "all64" else 1
            assert only_bits(mask, level, z0) and (cnt["recorded"], cnt["replay_steps"]) == (lanes, lanes)


def test_the_replay_ends_at_the_first_point_on_the_canvas(aref, ref):
    cases = P.replay_cases(ref)
    assert {t for *_, t in cases} >= {None, 1, 12, 13, 60, 61, 120, 121}
    for name, sample, end, box, t in cases:
        for shape in P.SHAPES:
            lanes = 64 if shape == "all64" else 1
            mask, cnt = probes(aref, P.lanes(sample, 64, shape), 6, box, end + 7, 0)
            # the fillers are accepted (min_iter 0), replay their one point, off the canvas, and mark nothing
            steps = lanes * (end if t is None else t) + (64 - lanes)
            assert cnt["replay_steps"] == steps and cnt["recorded"] == (0 if t is None else lanes), (name, shape, cnt)
            assert only_bits(mask, 6, *([] if t is None else [sample])), name
        if t is not None and t > 1:                                            # the neighbour: the canvas one point earlier
            earlier = P.box_from(P.orbit_of(ref, sample, end)[0][t - 2])
            _, other = probes(aref, P.lanes(sample), 6, earlier, end + 7, 0)
            assert other["replay_steps"] == t - 1 + 63


def test_samples_that_are_too_fast_never_escape_or_are_rejected_mark_nothing(aref, ref):
    (max_iter, min_iter), marker, others = P.unmarking_samples(ref)
    for level in (4, 10):
        assert all(P.mask_bit(level, *s) != P.mask_bit(level, *marker) for s in others)
        points = P.cycled([marker] + others, 64)
        mask, cnt = probes(aref, points, level, P.WIDE_BOX, max_iter, min_iter)
        n = points.count(marker)
        assert only_bits(mask, level, marker) and (cnt["recorded"], cnt["replay_steps"]) == (n, n)
        assert (cnt["too_fast"], cnt["never_escaped"], cnt["rejected"]) == tuple(
            points.count(s) for s in others[:2]) + (points.count(others[2]) + points.count(others[3]),)
        mask, cnt = probes(aref, P.cycled(others, 64), level, P.WIDE_BOX, max_iter, min_iter)
        assert not mask.any() and (cnt["recorded"], cnt["replay_steps"]) == (0, 0)


@pytest.mark.parametrize("case", P.BOUNDED_MARKS, ids=lambda c: c[0])
def test_the_bounded_probe_marks_at_the_first_point_of_transient_or_period(aref, ref, case):
    name, step, c, sample, box, t = case
    assert [f for f in P.repeating(ref, step, c) if f[0] == sample]            # a cycle the scheduler finds at 120
    m = P.BOUNDED_MAX_ITER
    for shape in P.SHAPES:
        lanes = 64 if shape == "all64" else 1
        for canvas, at in ((box, t), (P.NOWHERE, None)):                       # and no point at all: the full replay, no bit
            mask, cnt = probes(aref, P.lanes(sample, 64, shape), 6, canvas, m, 0, bounded=True, c=c, **step)
            m1, c1 = aim.probe(aref, mode=aim.COMPRESSED, states=P.plant_states(P.lanes(sample, 64, shape)), w=W, h=H,
                               box=canvas, max_iter=m, min_iter=0, threads=64, level=6, probe=(1,), bounded=True, c=c, **step)
            assert np.array_equal(m1, mask)
            assert {k: c1[k] for k in plot.COUNTER_NAMES} == {k: cnt[k] for k in plot.COUNTER_NAMES}
            assert (cnt["never_escaped"], cnt["too_fast"]) == (lanes, 64 - lanes)
            assert cnt["replay_steps"] == lanes * (m if at is None else at) and cnt["recorded"] == (0 if at is None else lanes)
            assert only_bits(mask, 6, *([] if at is None else [sample])), (name, canvas)
    if c is not None:
        assert P.mask_bit(6, *sample) != P.mask_bit(6, *c)
