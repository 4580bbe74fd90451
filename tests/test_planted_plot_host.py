"""The plants of the plotted renders (tests/planted_samples.py, the section on tests/plot_reference.py) shown decisive on
the restatement alone, no GPU: what tests/test_gpu_planted_plot.py and tests/test_gpu_planted_queue.py feed to the kernels
does sit on the decision it is named after.

  1. a planted `end` gives exactly the counters of planted_samples.model_counters, either side of max_iter and min_iter;
     a formula's planted orbit is another orbit under every other formula and under the two steps without one;
  2. the filler is decided at once under every step and source of c;
  3. the members of a slice pair put their increments into different planes, or in and out of the window;
  4. the members of a pixel pair put theirs into different pixels, or in and out of the canvas;
  5. a repeating orbit is seen to repeat from max_iter 121 on (the restatement compares z_120 with z_60 while 120 < max_iter;
     the scheduler does so at max_iter 120 too, where nothing is left to skip);
  6. a lone orbit under a palette adds weight_j of lut[end - 1] to plane j for each of its points on the canvas (all but
     the escaping one: end - 1 of them), and nothing under a zero entry;
  7. the frames queue, modelled: the fills the GPU cases claim.

THE FRAMES QUEUE'S LARGEST FILL IS 126.  With one sample per subsequence the fill before a drain cannot be 127: an append of
all 64 lanes needs every earlier contributor still replaying, so the total appended before it is 12 S + 64 (t - 1), which is
even and cannot be 63 mod 64.  The largest reachable fill is 63 left over and 63 appended, and that is planted."""

import numpy as np
import pytest

import bounded_reference as bounded
import frames_reference as frames
import planted_samples as P
import plot_reference as plot

W, H = 64, 48
STEPS = {"mandelbrot": {}, "ship": dict(ship=True), **P.POWER_STEPS, **P.FORMULA_STEPS}  # degrees 3 .. 8, the five formulas


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return plot.load(tmp_path_factory.mktemp("plot_ref"))


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return bounded.load(tmp_path_factory.mktemp("bounded_ref"))


def draw(ref, points, max_iter, min_iter, launches=(1,), extra=None, **kw):
    return plot.draw(ref, kw.pop("w", W), kw.pop("h", H), max_iter, min_iter, len(points), list(launches),
                     states=P.plant_states(points), extra=extra, **kw)


# ---- 1. and 2. ends and the filler -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("step", list(STEPS) + ["julia"])
def test_a_planted_end_is_that_end_and_gives_the_counters_of_the_model(ref, step):
    kw, c = ({}, P.FIXED_C) if step == "julia" else (STEPS[step], None)
    for end in P.ENDS:
        sample = P.with_end(ref, end, c, **kw)
        assert P.end_of(ref, sample, 200, c, **kw) == end
        for max_iter, min_iter, fate in P.windows_of(end):
            for shape in P.SHAPES:
                points = P.lanes(sample, 64, shape)
                n = sum(p == sample for p in points)
                model = P.model_counters([end if p == sample else 1 for p in points], max_iter, min_iter)
                _, wc = draw(ref, points, max_iter, min_iter, c=c, **kw)
                assert {k: wc[k] for k in model} == model, (step, end, max_iter, min_iter, shape)
                assert model[fate] >= n and (fate != "recorded" or model["replay_steps"] >= n * end)
                if min_iter >= 1:  # the fillers are idle: nothing but the planted lanes is replayed
                    assert model["replay_steps"] == (n * end if fate == "recorded" else 0)


def orbit_by_hand(ref, sample, n, **step):
    """z_1 .. z_n under plot.step, cut at the first escape: this file's own loop."""
    r, i = sample
    out = []
    for _ in range(n):
        r, i, m = plot.step(ref, sample[0], sample[1], r, i, **step)
        out.append(np.array([r, i]).tobytes())
        if m > 4.0:
            break
    return tuple(out)


@pytest.mark.parametrize("name", list(P.FORMULA_STEPS))
def test_a_formulas_planted_orbit_is_another_orbit_under_every_other_step(ref, name):
    """What makes a formula's plant decisive: up to its `end` the orbit of the planted sample differs bit for bit under every
    other formula, under the reference's step and under the Burning Ship's -- a kernel that took another branch of
    formula_step would visit other points.  One step has four classes only (P.FORMULA_RAYS): at end 1 the plant's z_1 is
    in another class than the steps with the other real part or the other sign of the cross term."""
    step = P.FORMULA_STEPS[name]
    others = [st for st in P.EVERY_STEP if st != step]
    assert len(others) == 6
    planted = {}
    for end in P.ENDS:
        sample = P.with_end(ref, end, **step)
        own = orbit_by_hand(ref, sample, end, **step)
        assert len(own) == end
        rest = [orbit_by_hand(ref, sample, end, **st) for st in others]
        if end > 1:
            assert own not in rest and len(set(rest)) == 6, (name, end)
            # every absolute value of the table decides somewhere: t < 0, z_re < 0 and z_im < 0 at points stepped from
            before = [sample] + [tuple(np.frombuffer(z)) for z in own[:-1]]
            assert any(r * r < i * i for r, i in before) and any(r < 0 and i != 0 for r, i in before), (name, end)
            assert any(i < 0 and r != 0 for r, i in before), (name, end)
        else:
            assert len({own, *rest}) == 4 == P.told_apart_at(1), (name, end)
        planted[end] = own
    # and the planted orbits themselves are not those of another formula's plants
    for other, st in P.FORMULA_STEPS.items():
        if other != name:
            for end in P.ENDS[1:]:
                assert orbit_by_hand(ref, P.with_end(ref, end, **st), end, **st) != planted[end]


def test_the_filler_is_decided_at_the_first_step_everywhere(ref):
    for kw in STEPS.values():
        for c in (None, P.FIXED_C, (-2.0, -2.0), (2.0, 2.0), (-2.0, 2.0), (-1.0, 0.0)):
            if c is None or not kw:
                assert P.end_of(ref, P.FILLER, 5, c, **kw) == 1
    assert not P.rejected(*P.FILLER) and P.rejected(0.0, 0.0)


# ---- 3. slices ------------------------------------------------------------------------------------------------------------

WINDOWS = P.SLICE_WINDOWS


@pytest.mark.parametrize("name", list(WINDOWS))
def test_slice_pairs_fall_into_different_planes(ref, name):
    lo, hi, n = WINDOWS[name]
    edges = P.slice_edges(ref, (lo, hi, n))
    pairs = edges["pairs"]
    assert [p[0] for p in pairs] == list(range(0 if lo > -2.0 else 1, n + 1))  # min = -2 has no plantable lower side
    assert pairs[-1][4] is None and pairs[-1][3] == n - 1 and (lo == -2.0 or (pairs[0][3] is None and pairs[0][4] == 0))
    assert (len(edges["disagree"]) > 0) == (name == "division_5")
    if n > 8:
        pairs = pairs[:2] + pairs[-2:]
    for j, below, above, sb, sa in pairs:
        assert above - below == P.GRID and sb != sa
        c_im, ends = P.accepted_beside(ref, (below, above))
        for c_re, s, end in ((below, sb, ends[0]), (above, sa, ends[1])):
            hist, wc = draw(ref, P.lanes((c_re, c_im)), 500, 1, depth=("cr", lo, hi, n), box=P.WIDE_BOX)
            plain, pc = draw(ref, P.lanes((c_re, c_im)), 500, 1, box=P.WIDE_BOX)
            assert wc["replay_steps"] == end and pc["increments"] > 0
            if s is None:
                assert wc["increments"] == 0
            else:
                assert int(hist[s].sum()) == wc["increments"] == pc["increments"] and np.array_equal(hist[s], plain)
    for c_re, s, other in edges["disagree"]:  # the reciprocal would name another slice: the division decides
        assert s != other and s is not None
        c_im, _ = P.accepted_beside(ref, (c_re,))
        hist, wc = draw(ref, P.lanes((c_re, c_im)), 500, 1, depth=("cr", lo, hi, n), box=P.WIDE_BOX)
        assert int(hist[s].sum()) == wc["increments"] > 0


# ---- 4. pixels --------------------------------------------------------------------------------------------------------------

C_BOX = P.C_BOX


def test_c_plane_pairs_fall_into_different_pixels(ref):
    seen = set()
    for axis, name, on, below in P.c_plane_edges(C_BOX, W, H):
        n = (W, H)[axis]
        want = {"min": (0, None), "inner": (n // 3, n // 3 - 1), "max": (None, n - 1)}[name]
        for coordinate, index in zip((on, below), want):
            sample = P.c_plane_sample(axis, coordinate)
            end = P.end_of(ref, sample, 200)
            assert end >= 2 and not P.rejected(*sample)
            assert plot.point(ref, plot.C_PLANE, 0.3, -0.7, *sample) == sample  # (u, v) is c exactly, whatever z
            hist, wc = draw(ref, P.lanes(sample), 1000, 1, projection=plot.C_PLANE, box=C_BOX)
            assert wc["recorded"] == 1 and wc["replay_steps"] == end
            if index is None:
                assert wc["increments"] == 0
            else:
                row, col = np.argwhere(hist)[0]
                assert int(hist[row, col]) == end == wc["increments"] and (col, row)[axis] == index
                seen.add((axis, name, index))
    assert len(seen) == 8


def test_hologram_canvases_put_an_orbit_point_on_their_borders(ref):
    sample, (u, v), canvases = P.hologram_canvases(ref, W, H)
    counts = {}
    for kind in ("on_min", "below_min", "on_max"):
        (box,) = canvases[kind]
        hist, wc = draw(ref, P.lanes(sample), 61, 1, projection=plot.HOLOGRAM, box=box)
        assert wc["recorded"] == 1 and np.array_equal(hist, P.histogram(box, W, H, u, v))
        counts[kind] = wc["increments"]
    assert counts["on_min"] > counts["below_min"]  # the points on the two lower bounds are counted, one ulp below not


# ---- 5. repeating orbits ----------------------------------------------------------------------------------------------------


def test_repeating_orbits_repeat_and_are_seen_from_121(ref, bref):
    kept = 0
    for step, c, _ in P.REPEATING:
        for sample, period, on_circle in P.repeating(ref, step, c):
            kept += 1
            assert on_circle == (c == (-2.0, 0.0))
            for max_iter in (119, 120, 121, 180):
                extra = {}
                _, wc = draw(ref, P.lanes(sample, shape="all64"), max_iter, 1, c=c, extra=extra, reject=False, **step)
                assert wc["never_escaped"] == 64 and wc["recorded"] == 0
                assert extra["chunk_repeats"] == (64 if max_iter > 120 else 0)
            for max_iter in (120, 121, 179, 180, 181):  # bounded: s = 60, p = 60, rem = (max_iter - 60) % 60
                ex = {}
                hist, bc = bounded.draw(bref, W, H, max_iter, 64, [1], states=P.plant_states(P.lanes(sample)), c=c,
                                        box=P.WIDE_BOX, mode=bounded.COMPRESSED, extra=ex, **step)
                assert ex["cycles"] == 1 and ex["escaped"] == 63 and bc["increments"] == max_iter == int(hist.sum())
                assert ex["rem_zero"] == (max_iter % 60 == 0) and ex["at_m"] == (max_iter == 120)
                assert bc["skipped_steps"] == (max_iter - 120) + (max_iter - 119)
    assert kept >= len(P.REPEATING)


# ---- 6. palette -------------------------------------------------------------------------------------------------------------


def test_a_lone_orbit_under_a_palette_adds_its_entry(ref):
    max_iter, min_iter = 61, 12
    lut = plot.demo_table(max_iter)
    assert len({int(lut[k]) for k in (11, 12, 13, 59, 60)}) == 5
    for end, fate in ((12, "too_fast"), (13, "recorded"), (61, "recorded"), (62, "never_escaped")):
        sample = P.with_end(ref, end)
        hist, wc = draw(ref, P.lanes(sample), max_iter, min_iter, lut=lut)
        plain, pc = draw(ref, P.lanes(sample), max_iter, min_iter)
        assert wc[fate] >= 1 and wc["recorded"] == (fate == "recorded")
        if fate == "recorded":
            assert pc["increments"] == end - 1  # all of the orbit but the escaping point is on the canvas
            assert [int(p.sum()) for p in hist] == [(end - 1) * int(w) for w in plot.weights(lut)[end - 1]]
            assert all(np.array_equal(p, plain * w) for p, w in zip(hist, plot.weights(lut)[end - 1]))
            for zero in (0, 0xAB000000):
                table = lut.copy()
                table[end - 1] = zero
                extra = {}
                hist, wc = draw(ref, P.lanes(sample), max_iter, min_iter, lut=table, extra=extra)
                assert not hist.any() and wc["recorded"] == 1 and extra["zero_entry_steps"] == end
        else:
            assert not hist.any()


# ---- 7. the frames queue ----------------------------------------------------------------------------------------------------


def test_the_queue_model_gives_the_fills_the_gpu_cases_claim():
    assert P.queue_fills([13] * 64) == ([64] * 13, 0)                       # 64 lanes in phase: 64 at every hook
    assert P.queue_fills([61] * 64) == ([64] * 61, 0)
    fills, rest = P.queue_fills([13] * 63 + [1])                            # 63 in phase and a filler
    assert max(fills) == 126 and fills[0] == 126 and rest == 13 * 63 - 12 * 64
    assert P.queue_fills([1] + [None] * 63, min_iter=0) == ([], 1)          # a one-point orbit: 1 at `last`
    assert P.queue_fills([1] * 63 + [None], min_iter=0) == ([], 63)         # 63 of them: 63 at `last`
    assert P.queue_fills([2] * 63 + [1]) == ([126], 62)
    # no fill of 127 with one sample per lane: every fill of every mix of these ends is at most 126
    rng = np.random.default_rng(5)
    for _ in range(200):
        ends = [int(e) if e else None for e in rng.choice([0, 2, 12, 13, 24, 25, 61], size=64)]
        fills, rest = P.queue_fills(ends)
        assert all(64 <= f <= 126 for f in fills) and 0 <= rest <= 63


def test_frames_of_a_lone_orbit_are_its_plain_renders(ref):
    sample = P.with_end(ref, 13)
    mats = [plot.IDENTITY, plot.C_PLANE, plot.HOLOGRAM]
    hist, wc = frames.draw(ref, mats, W, H, 13, 1, 64, [1], states=P.plant_states(P.lanes(sample)))
    assert wc["recorded"] == 1 and wc["replay_steps"] == 13 and int(hist[1].max()) == 13 == int(hist[1].sum())
