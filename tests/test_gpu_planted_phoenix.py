"""The Phoenix render's kernels (draw_phoenix.hip: the product kernel, cb_debug_last_draw_kernel 24, run_rounds with
PhoenixMode and its three state hooks start, save and same; the lock-step kernel, 25) on PLANTED samples: the first sample
of every subsequence is chosen to the bit (tests/planted_samples.py) --

  a. an orbit that escapes at a round's or a chunk's last step or the next one's first, either side of max_iter and
     min_iter, alone in lane 0, alone in lane 63, in all 64 lanes;
  b. every such end cycled through two blocks and followed by the generators' own samples (the sample after a planted orbit
     starts from y = 0: `start` in ITERATE);
  c. an orbit that returns to its saved z bit for bit at one chunk and to its saved state (z, y) only at a later one, or
     never: skipped_steps is the state rule's discount to the step, after the first save and after later ones (`save`,
     `same`), and per lane;
  d. an orbit with |z|^2 == 4.0 exactly (the strict test keeps it);
  e. a hand-computed orbit whose replayed points move if REPLAY does not start from y = 0 (`start` in REPLAY);
  f. p = 0 on planted states: the projected render without rejection, and the Julia kernels;
  g. parameters and a fixed c whose zeros are negative.

The generators' own samples reach none of these to the step; tests/test_planted_phoenix_host.py shows on the restatement
alone that the planted ones do.  Every case is phoenix_harness.three_ways on planted states: product == lock-step ==
restatement, bit for bit on histogram, the counters of SAME and the generator states after the run, status 0, and the
product's skipped_steps == the restatement's discount under the state rule; where the host file derives a figure it is
asserted on the device's counters too.  64 subsequences, or 512; launches of one sample and once (1, 50); 64 x 48;
max_iter at most 1000."""

import numpy as np
import pytest

import phoenix_harness
import phoenix_reference as phoenix
import planted_samples as P
import plot_harness
import plot_reference as plot
from plot_harness import SAME, SQUARE, omp_threads
from plot_harness import ref  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

W, H = 64, 48
PRODUCT, LOCKSTEP = phoenix_harness.PRODUCT, phoenix_harness.LOCKSTEP
ZERO = (0.0, 0.0)


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return phoenix.load(tmp_path_factory.mktemp("phoenix_ref"))


@pytest.fixture(scope="module")
def found(pref):
    """The searches, once for the module: found("ends", setting) -> [(end, sample)]; found("cycle", k) -> (found_z,
    found_state) of P.PHOENIX_CYCLES[k]."""
    done = {}

    def get(kind, key):
        if (kind, key) not in done:
            if kind == "ends":
                p, c = {**P.PHOENIX_SETTINGS, **P.PHOENIX_BOUNDS}[key]
                done[kind, key] = P.ends_found(pref, c, phoenix=p)
            else:
                p, c, sample = P.PHOENIX_CYCLES[key]
                ((_, found_z, found_state),) = P.phoenix_cycles(pref, p, c, [(p, c, sample)])
                done[kind, key] = (found_z, found_state)
        return done[kind, key]

    return get


def three(cb, pref, oracle, points, max_iter, min_iter, p, c=None, launches=(1,), box=SQUARE):
    """phoenix_harness.three_ways on planted first samples, at this suite's canvas -> (hist, counters, extra, product)."""
    return phoenix_harness.three_ways(cb, pref, oracle, states=P.plant_states(points), w=W, h=H, box=box, max_iter=max_iter,
                                      min_iter=min_iter, threads=len(points), launches=launches, p=p, c=c)


# ---- a. ends at round and chunk edges -----------------------------------------------------------------------------------------


def ends_either_side_of_the_window(cb, pref, oracle, p, c, end, sample):
    for max_iter, min_iter, fate in P.windows_of(end):
        for shape in P.SHAPES:
            points = P.lanes(sample, 64, shape)
            _, _, _, product = three(cb, pref, oracle, points, max_iter, min_iter, p, c)
            model = P.model_counters([end if q == sample else 1 for q in points], max_iter, min_iter)
            assert {k: product[k] for k in model} == model, (p, c, end, max_iter, min_iter, shape)
            assert product["skipped_steps"] == 0


@pytest.mark.parametrize("end", P.ENDS)
@pytest.mark.parametrize("setting", list(P.PHOENIX_SETTINGS))
def test_an_escape_at_a_round_or_chunk_edge_either_side_of_the_window(cb, pref, oracle, found, setting, end):
    """`end` = 1, 12, 13, 60, 61, 120, 121 against kRound = 12 and kChunk = 60, with k = end - 1 the last k accepted
    (max_iter = end), never escaping (max_iter = end - 1), accepted (min_iter = end - 1) and too fast (min_iter = end)."""
    p, c = P.PHOENIX_SETTINGS[setting]
    (sample,) = [s for e, s in found("ends", setting) if e == end]
    ends_either_side_of_the_window(cb, pref, oracle, p, c, end, sample)


@pytest.mark.parametrize("setting", list(P.PHOENIX_BOUNDS))
def test_the_ends_there_are_at_the_bounds_of_p(cb, pref, oracle, found, setting):
    p, c = P.PHOENIX_BOUNDS[setting]
    ends = found("ends", setting)
    assert {e for e, _ in ends} >= set(P.BOUND_ENDS)
    for end, sample in ends:
        ends_either_side_of_the_window(cb, pref, oracle, p, c, end, sample)


# ---- b. planted ends, then the generators' own samples ----------------------------------------------------------------------------


@pytest.mark.parametrize("setting", list(P.PHOENIX_SETTINGS))
def test_planted_ends_followed_by_the_generators_own_samples(cb, pref, oracle, found, setting):
    """Every end of the list, cycled through 512 subsequences (two whole blocks), then 50 samples of the generators' own:
    the sample after a planted orbit, iterated or replayed, begins with y = 0."""
    p, c = P.PHOENIX_SETTINGS[setting]
    points = P.cycled([s for _, s in found("ends", setting)], 512)
    _, wc, _, _ = three(cb, pref, oracle, points, 121, 12, p, c, (1, 50))
    assert wc["recorded"] > 512 * 4 // 7


# ---- c. the state rule, to the step -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", range(len(P.PHOENIX_CYCLES)), ids=lambda k: "%d" % k)
def test_the_cycle_is_found_where_the_whole_state_repeats(cb, pref, oracle, found, case):
    """z_k == z_saved at found_z with another y: the orbit goes on.  The product kernel retires the sample at found_state,
    against the state saved last -- after 1, 2, 3 or 4 chunks --, and skips max_iter - found_state steps where found_state <
    max_iter; under the z-only rule the figure would be max_iter - found_z."""
    p, c, sample = P.PHOENIX_CYCLES[case]
    found_z, found_state = found("cycle", case)
    for max_iter in P.cycle_max_iters(found_z, found_state):
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            _, wc, extra, product = three(cb, pref, oracle, points, max_iter, 1, p, c)
            assert product["never_escaped"] == n and product["too_fast"] == 64 - n and product["recorded"] == 0
            assert product["skipped_steps"] == n * P.cycle_discount(found_state, max_iter)
            z_only = n * P.cycle_discount(found_z, max_iter)
            assert extra["skipped_z_only"] == z_only
            assert (product["skipped_steps"] != z_only) == (max_iter > found_z)


def test_save_and_same_are_per_lane(cb, pref, oracle, found):
    """Two plants of one setting alternating lane by lane in one wave, found at different chunks: the sum of their discounts."""
    (p, c, a), (_, _, b) = P.PHOENIX_CYCLES[0], P.PHOENIX_CYCLES[1]
    (_, state_a), (_, state_b) = found("cycle", 0), found("cycle", 1)
    assert (p, c) == P.PHOENIX_CYCLES[1][:2] and state_a != state_b
    for max_iter in (state_a + 1, state_b + 1, 300):
        _, _, _, product = three(cb, pref, oracle, P.cycled([a, b], 64), max_iter, 1, p, c)
        assert product["never_escaped"] == 64
        assert product["skipped_steps"] == 32 * P.cycle_discount(state_a, max_iter) + 32 * P.cycle_discount(state_b, max_iter)


# ---- d. on the circle -----------------------------------------------------------------------------------------------------------


def test_a_point_on_the_circle_has_not_escaped(cb, pref, oracle):
    """|z|^2 == 4.0 exactly under the strict test: the sampled plant is recorded with two points, not one; the fixed one never
    escapes."""
    p, c, sample, _, end = P.PHOENIX_CIRCLE["sampled"]
    for max_iter in (2, 3, 121):
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            want, _, _, product = three(cb, pref, oracle, points, max_iter, 1, p, c, box=P.WIDE_BOX)
            assert product["recorded"] == n and product["replay_steps"] == end * n == 2 * n
            assert np.array_equal(want, P.histogram(P.WIDE_BOX, W, H, [2.0], [0.0]) * np.uint64(n))  # z_1 = 2; 4.5 is off it
    _, _, _, product = three(cb, pref, oracle, P.lanes(sample), 1, 0, p, c, box=P.WIDE_BOX)
    assert product["never_escaped"] == 1 and product["recorded"] == 63  # max_iter 1: only the fillers' z_1 escapes
    p, c, sample, _, end = P.PHOENIX_CIRCLE["fixed"]
    assert end is None
    for max_iter in (3, 4, 121):
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            _, _, _, product = three(cb, pref, oracle, points, max_iter, 1, p, c, box=P.WIDE_BOX)
            assert product["never_escaped"] == n and product["recorded"] == 0 and product["too_fast"] == 64 - n
            assert product["iterate_steps"] == n * max_iter + 64 - n


# ---- e. replay starts from y = 0 ------------------------------------------------------------------------------------------------


def test_a_replay_starts_from_y_zero(cb, pref, oracle, found):
    """ITERATE leaves y = z_{end - 1}; REPLAY must begin with y = 0 again.  The hand-computed plant, and a found one of 13
    points: the histogram is that of orbit_of's points, once per lane that holds the orbit."""
    r = P.PHOENIX_REPLAY
    p, c = P.PHOENIX_SETTINGS["sampled"]
    (long_sample,) = [s for e, s in found("ends", "sampled") if e == 13]
    for sample, pp, end, given in ((r["sample"], r["p"], r["end"], r["points"]), (long_sample, p, 13, None)):
        orbit, got = P.orbit_of(pref, sample, end, phoenix=pp)
        assert got == end and (given is None or orbit == given)
        one = P.histogram(P.WIDE_BOX, W, H, *zip(*orbit))
        assert int(one.sum()) >= end - 1
        for shape in P.SHAPES:
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            want, _, _, product = three(cb, pref, oracle, points, end, 1, pp, box=P.WIDE_BOX)
            assert np.array_equal(want, one * np.uint64(n))
            assert product["recorded"] == n and product["replay_steps"] == n * end and product["increments"] == n * int(one.sum())


# ---- f. p = 0 -------------------------------------------------------------------------------------------------------------------


def test_p_zero_on_planted_states_is_the_projected_render_without_rejection(cb, pref, ref, oracle):  # noqa: F811
    points = P.cycled([P.with_end(ref, end) for end in P.ENDS], 512)
    want, wc, _, _ = three(cb, pref, oracle, points, 121, 12, ZERO, None, (1, 50))
    st = P.plant_states(points)
    hist, pc = plot.draw(ref, W, H, 121, 12, 512, [1, 50], reject=False, states=st, omp_threads=omp_threads())
    assert pc["rejected"] == 0 and pc["recorded"] > 512 * 4 // 7
    assert wc == pc and np.array_equal(want, hist)


def test_p_zero_with_a_fixed_c_on_planted_states_is_the_julia_render(cb, pref, ref, oracle):  # noqa: F811
    c = P.FIXED_C
    points = P.cycled([P.with_end(ref, end, c) for end in P.ENDS], 512)
    want, wc, _, _ = three(cb, pref, oracle, points, 121, 12, ZERO, c, (1, 50))
    assert wc["recorded"] > 512 * 4 // 7
    states = P.plant_states(points)
    after = phoenix_harness.restated(pref, oracle, states, w=W, h=H, max_iter=121, min_iter=12, threads=512, launches=(1, 50),
                                     p=ZERO, c=c)[3]
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, 12), (cb.CB_KERNEL_SIMPLE, 13)):
        jh, jc, launched, js = plot_harness.gpu_launches(cb, W, H, SQUARE, 121, 12, 512, (1, 50), base, c, states=states)
        assert launched == kernel and jc["status"] == 0
        assert np.array_equal(jh, want) and np.array_equal(js, after)
        assert {k: jc[k] for k in SAME} == wc


# ---- g. negative zeros -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(P.PHOENIX_ZEROS))
def test_negative_zeros_in_p_and_c(cb, pref, oracle, name):
    """The cycle test compares bits: +0 and -0 differ.  Product, lock-step and restatement give the zeros the same signs, so
    the state is found where the restatement finds it."""
    p, c, sample = P.PHOENIX_ZEROS[name]
    ((_, found_z, found_state),) = P.phoenix_cycles(pref, p, c, [(p, c, sample)])
    assert found_z == found_state
    for max_iter in P.ZEROS_MAX_ITERS:
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            _, _, extra, product = three(cb, pref, oracle, points, max_iter, 1, p, c, box=P.WIDE_BOX)
            assert product["never_escaped"] == n and product["recorded"] == 0
            assert product["skipped_steps"] == extra["skipped_state"] == n * P.cycle_discount(found_state, max_iter)
