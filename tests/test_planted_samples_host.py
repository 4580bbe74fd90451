"""tests/planted_samples.py on the reference alone: the states it makes draw what was asked, and the samples and canvases
its finders return are DECISIVE -- a neighbour one grid step or one iteration away changes an oracle counter, and a
histogram binned with the quotient's estimate alone differs from the oracle's.  tests/test_gpu_planted_samples.py gives
the same inputs to the draw kernels; what it can catch is what is shown here."""

import numpy as np
import pytest

import planted_samples as P

W, H = 333, 300


def draw_one(oracle, point, max_iter, min_iter, box=(-2.0, 2.0, -2.0, 2.0), w=16, h=16):
    """The planted sample alone through DrawBuddhabrot -> (hist, counters)."""
    states = P.plant_states([point])
    return oracle.render(w, h, max_iter, min_iter, 1, 1, box, samples_per_thread=1, states=states)


def test_plant_state_round_trips_over_the_grid():
    """A few thousand grid points, the grid's two ends and zero among them, with every free word varied; -2 and points
    off the grid are refused."""
    rng = np.random.default_rng(11)
    ends = [(1 << 52), -(1 << 52) + 1, 0, 1, -1, (1 << 52) - 1, 1 << 32, (1 << 32) - 1, -(1 << 32)]
    steps = ends + [int(v) for v in rng.integers(-(1 << 52) + 1, (1 << 52) + 1, 3000)]
    points = [(P.grid_point(a), P.grid_point(b)) for a, b in zip(steps, reversed(steps))]
    assert points[0][0] == 2.0 and points[1][0] == -2.0 + P.GRID and points[2][0] == 0.0
    assert all(P._f_inverse(P._f(v)) == v == P._f(P._f_inverse(v)) for v in [0, 1, P.M32, 1 << 31] + [n & P.M32 for n in steps[9:209]])
    states = P.plant_states(points, salt=3)            # plant_state asserts orc_uniform_double's answer for each
    for k in (0, 1, 2, 17, 3008):
        assert P.first_sample(states[k]) == points[k]
    assert len({int(s["d"]) for s in states}) > 3000 and len({int(s["x"][4]) for s in states}) > 3000
    for bad in (-2.0, 2.0 + 2.0 ** -50, 2.0 ** -52, 0.1):
        with pytest.raises(ValueError):
            P.plant_state(bad, 0.0)


def test_the_generator_goes_on_by_itself_after_the_planted_sample(oracle):
    """One planted sample per subsequence: the second sample is not ours, differs from lane to lane, and the oracle
    counts 50 samples from such a state like from any other."""
    states = P.plant_states([(0.25, 0.5)] * 64)
    _, cnt = oracle.render(8, 8, 50, 5, 64, 1, states=states.copy())
    assert cnt["samples"] == 64 * 50
    seconds = set()
    for k in range(64):
        one = states[k:k + 1].copy()
        oracle.render(8, 8, 50, 5, 1, 1, samples_per_thread=1, states=one)     # draws the planted sample
        seconds.add(P.first_sample(one[0]))
    assert len(seconds) == 64


@pytest.mark.parametrize("ray", ["cusp", "neck"])
def test_mandel_orbit_is_the_oracles_step(oracle, ray):
    """The Python step against orc_iterate_mandelbrot's count, and its points against IterateAndRecord's histogram."""
    for n in (1, 2, 19, 20, 61, 300, 1233):
        c = P.with_escape_count(n, ray)
        rs, is_, count = P.mandel_orbit(*c, n + 5)
        assert count == n == P.escape_count(*c, n + 5) and len(rs) == n + 1
        box = (-1.7, 0.9, -0.3, 1.1)
        want, steps, incr = oracle.record_points(W, 77, box, [c[0]], [c[1]])
        got = P.histogram(box, W, 77, rs, is_)
        assert steps == n + 1 and np.array_equal(got, want) and int(got.sum()) == incr
    rs, is_, count = P.mandel_orbit(0.3, 0.0, 50)
    assert np.array_equal(rs, P.real_axis_orbits(np.array([0.3]), len(rs))[:, 0]) and not is_.any()


@pytest.mark.parametrize("window", P.WIDE_WINDOWS + P.PROBE_WINDOWS, ids=lambda w: "%d_%d" % w)
def test_escape_count_cases_are_exact_and_neighbours_differ(oracle, window):
    """Every planted count is the oracle's count, and the samples either side of min_iter and of max_iter end in
    different counters: too_fast | recorded, recorded | never_escaped."""
    max_iter, min_iter = window
    fate = {}
    for count, c in P.window_samples(max_iter, min_iter):
        assert P.escape_count(*c, max_iter + 5) == count
        _, cnt = draw_one(oracle, c, max_iter, min_iter)
        want = P.expected_fate(count, max_iter, min_iter)
        assert cnt[want] == 1 and cnt["samples"] == 1 and cnt["rejected"] == 0, (count, cnt)
        assert cnt["iterate_steps"] == min(count + 1, max_iter)
        fate.setdefault(count, set()).add(want)
    assert fate[min_iter - 1] == {"too_fast"} and fate[min_iter] == {"recorded"}
    assert fate[max_iter - 1] == {"recorded"} and fate[max_iter] == {"never_escaped"} == fate[max_iter + 1]
    long_start, tail_start = P.stage_plan(max_iter, min_iter)
    assert {long_start, long_start + P.CHUNK, tail_start - 1, tail_start + 1} <= set(fate)


@pytest.mark.parametrize("shape", ["cardioid", "bulb"])
def test_shape_pairs_differ_in_rejected(oracle, shape):
    pairs = P.cardioid_pairs() if shape == "cardioid" else P.bulb_pairs()
    assert len(pairs) >= 20
    test = oracle.lib.orc_in_main_cardioid if shape == "cardioid" else oracle.lib.orc_in_order2_bulb
    for inside, outside in pairs:
        assert test(*inside) and not test(*outside)
        steps = [abs(P.grid_index(a) - P.grid_index(b)) for a, b in zip(inside, outside)]
        assert sorted(steps) == [0, 1]                                      # neighbours on the grid, along one axis
        _, a = draw_one(oracle, inside, 100, 20)
        _, b = draw_one(oracle, outside, 100, 20)
        assert (a["rejected"], b["rejected"]) == (1, 0) and a["iterate_steps"] == 0 < b["iterate_steps"]
    # the spread the suite asks for: both signs of imag, the axis, the cusp, and -3/4 where the shapes touch
    ims = [p[0][1] for p in pairs]
    assert min(ims) < 0 < max(ims) and 0.0 in ims
    assert any(abs(p[1][0] + 0.75) < 1e-6 and abs(p[1][1]) < 1e-3 for p in pairs)
    if shape == "cardioid":
        assert ((0.25 - P.GRID, 0.0), (0.25, 0.0)) in pairs
        assert ((-0.75 + P.GRID, 0.0), (-0.75, 0.0)) in pairs
    else:
        assert ((-0.75 - P.GRID, 0.0), (-0.75, 0.0)) in pairs and ((-1.25 + P.GRID, 0.0), (-1.25, 0.0)) in pairs


@pytest.fixture(scope="module")
def edge_cases():
    """The pixel-edge inputs of the GPU suite: its base orbit, the canvases found for it, and per canvas the further
    samples on the real axis."""
    return P.pixel_edge_cases(W, H)


def test_pixel_edge_canvases_need_the_exact_division(oracle, edge_cases):
    """On every canvas at least 8 distinct orbit points are binned differently by the estimate alone -- in columns and in
    rows --, every one of them fails the kernels' guard (edge_disagreements asserts it), the quotient's histogram is the
    oracle's and the estimate's is not."""
    base, canvases = edge_cases
    assert len(canvases["fallback"]) >= 2
    for box, samples in canvases["fallback"]:
        assert len(set(samples)) == len(samples) and base in samples
        dr, di = P.deltas(box, W, H)
        assert all(np.frexp(d)[0] != 0.5 for d in (dr, di)), "a dyadic pixel side never divides"
        rs, is_, cols, rows = [], [], 0, 0
        for c in samples:
            r, i, count = P.mandel_orbit(*c, 1234)
            assert 20 <= count < 1234
            idx = P.edge_disagreements(box, W, H, r, i)
            cq, rq, _ = P.pixels(box, W, H, r, i)
            ce, re_, _ = P.pixels(box, W, H, r, i, estimate=True)
            cols += int(np.count_nonzero(cq[idx] != ce[idx]))
            rows += int(np.count_nonzero(rq[idx] != re_[idx]))
            assert len(idx) >= 1
            rs.append(r)
            is_.append(i)
        assert cols + rows >= 8 and cols >= 1 and rows >= 1, (box, cols, rows)
        rs, is_ = np.concatenate(rs), np.concatenate(is_)
        want, steps, incr = oracle.record_points(W, H, box, [c[0] for c in samples], [c[1] for c in samples])
        assert steps == len(rs)
        assert np.array_equal(P.histogram(box, W, H, rs, is_), want)
        wrong = P.histogram(box, W, H, rs, is_, estimate=True)
        assert not np.array_equal(wrong, want)
        assert int(np.abs(wrong.astype(np.int64) - want.astype(np.int64)).sum()) >= 8


def test_canvas_border_cases_are_what_they_claim(oracle, edge_cases):
    """A point exactly on min is counted in pixel 0 and fails the guard (its estimate is 0); one ulp below it is not
    counted; a point exactly on max is counted or not as the oracle's own division says."""
    base, canvases = edge_cases
    rs, is_, _ = P.mandel_orbit(*base, 1234)

    def increments(box):
        hist, _, incr = oracle.record_points(W, H, box, [base[0]], [base[1]])
        assert np.array_equal(hist, P.histogram(box, W, H, rs, is_))
        return hist, incr

    (on,), (below,), (top,) = canvases["on_min"], canvases["below_min"], canvases["on_max"]
    hist, n_on = increments(on)
    col, row, ok = P.pixels(on, W, H, rs, is_)
    assert np.any(ok & (rs == on[0]) & (col == 0)) and np.any(ok & (is_ == on[2]) & (row == 0))
    _, n_below = increments(below)
    _, _, ok_below = P.pixels(below, W, H, rs, is_)
    assert not np.any(ok_below & ((rs == on[0]) | (is_ == on[2]))) and n_below < n_on
    _, n_top = increments(top)
    assert np.any(rs == top[1]) and np.any(is_ == top[3]) and n_top > 0
    dr, di = P.deltas(top, W, H)
    col, row, ok = P.pixels(top, W, H, rs, is_)
    for z, lo, hi, d, n, pix in ((rs, top[0], top[1], dr, W, col), (is_, top[2], top[3], di, H, row)):
        q = int((hi - lo) / d)                              # the reference's own conversion
        assert q in (n - 1, n)
        assert np.all((pix[z == hi] == n - 1) if q == n - 1 else ~ok[z == hi])


def test_the_real_samples_serve_the_burning_ship_too(oracle, edge_cases):
    """|re|, |im| before every step change nothing on a positive real orbit: the real samples of the first canvas have the
    same points under the RENDER_BURNING_SHIP step (restated by mandel_orbit(ship=True)), the oracle's ship build bins them
    like the quotient, and the estimate alone still gets at least 8 of them wrong."""
    _, canvases = edge_cases
    box, samples = canvases["fallback"][0]
    real = samples[1:]
    rs, is_ = [], []
    for c in real:
        r, i, count = P.mandel_orbit(*c, 1234, ship=True)
        plain = P.mandel_orbit(*c, 1234)
        assert np.array_equal(r, plain[0]) and np.array_equal(i, plain[1]) and count == plain[2] and np.all(r > 0)
        rs.append(r)
        is_.append(i)
    rs, is_ = np.concatenate(rs), np.concatenate(is_)
    oracle.lib.orc_set_burning_ship(1)
    try:
        want, steps, _ = oracle.record_points(W, H, box, [c[0] for c in real], [c[1] for c in real])
    finally:
        oracle.lib.orc_set_burning_ship(0)
    assert steps == len(rs) and np.array_equal(P.histogram(box, W, H, rs, is_), want)
    assert len(P.edge_disagreements(box, W, H, rs, is_)) >= 8
