"""The plants of the Phoenix render (tests/planted_samples.py, "the cases both Phoenix suites use") shown decisive on the
restatement alone (tests/phoenix_reference.c), no GPU: what tests/test_gpu_planted_phoenix.py feeds to kernels 24 and 25
does sit on the decision it is named after.

  1. a planted `end` is that end, recomputed here step by step, and gives exactly the counters of
     planted_samples.model_counters either side of max_iter and min_iter -- every end of P.ENDS under the three main
     settings, the ends the rays have (1, 12 and 13 at the least) at the bounds of p; the filler is decided at once;
  2. a cycle plant is found by z alone at one chunk and by the whole state at a later one or never, the two discounts of the
     restatement are n * max(max_iter - found, 0) each and differ exactly where max_iter is beyond the first; the search
     that the later candidates came from finds them again;
  3. the circle plants have |z|^2 == 4.0 exactly at the steps named and the `end` stated;
  4. the replay plant's hand-computed points are the restatement's, under another projection too, and a replay that kept
     ITERATE's y would leave them;
  5. p = 0 is the Mandelbrot step without rejection, on the planted states;
  6. the negative-zero plants are what their comment says.
"""

import numpy as np
import pytest

import phoenix_reference as phoenix
import planted_samples as P
import plot_reference as plot

W, H = 64, 48
SETTINGS = {**P.PHOENIX_SETTINGS, **P.PHOENIX_BOUNDS}


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return phoenix.load(tmp_path_factory.mktemp("phoenix_ref"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return plot.load(tmp_path_factory.mktemp("plot_ref"))


def draw(pref, points, max_iter, min_iter, p, c=None, launches=(1,), box=(-2.0, 2.0, -2.0, 2.0), extra=None):
    return phoenix.draw(pref, W, H, max_iter, min_iter, len(points), list(launches), p=p, c=c, box=box,
                        states=P.plant_states(points), extra=extra)


def end_by_hand(pref, sample, p, c, cap):
    """The first k with |z_k|^2 > 4 among z_1 .. z_cap, from (z_0, y_0 = 0): this file's own loop on the step."""
    cr, ci = sample if c is None else c
    state = (sample[0], sample[1], 0.0, 0.0)
    for k in range(1, cap + 1):
        *state, m = phoenix.step(pref, cr, ci, p[0], p[1], *state)
        if m > 4.0:
            return k
    return None


# ---- 1. ends and the filler ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_planted_end_is_that_end_and_gives_the_counters_of_the_model(pref, setting):
    p, c = SETTINGS[setting]
    found = P.ends_found(pref, c, phoenix=p)
    ends = [end for end, _ in found]
    if setting in P.PHOENIX_SETTINGS:
        assert ends == list(P.ENDS)
    else:
        assert set(ends) >= set(P.BOUND_ENDS)
    for end, sample in found:
        P.grid_index(sample[0]), P.grid_index(sample[1])
        assert end_by_hand(pref, sample, p, c, 200) == end
        for max_iter, min_iter, fate in P.windows_of(end):
            for shape in P.SHAPES:
                points = P.lanes(sample, 64, shape)
                n = sum(q == sample for q in points)
                model = P.model_counters([end if q == sample else 1 for q in points], max_iter, min_iter)
                extra = {}
                _, wc = draw(pref, points, max_iter, min_iter, p, c, extra=extra)
                assert {k: wc[k] for k in model} == model, (setting, end, max_iter, min_iter, shape)
                assert model[fate] >= n and extra["skipped_state"] == 0
                if min_iter >= 1:  # the fillers are idle: nothing but the planted lanes is replayed
                    assert model["replay_steps"] == (n * end if fate == "recorded" else 0)


def test_the_filler_is_decided_at_the_first_step_under_every_setting(pref):
    settings = list(SETTINGS.values()) + [v[:2] for v in P.PHOENIX_CIRCLE.values()] + [v[:2] for v in P.PHOENIX_ZEROS.values()]
    settings += [(pp, cc) for pp, cc, _ in P.PHOENIX_CYCLES] + [(P.PHOENIX_REPLAY["p"], None), ((0.0, 0.0), None),
                                                                ((0.0, 0.0), P.FIXED_C)]
    for p, c in settings:
        assert end_by_hand(pref, P.FILLER, p, c, 5) == 1


# ---- 2. cycles ------------------------------------------------------------------------------------------------------------------


def test_every_cycle_candidate_is_confirmed_and_both_kinds_are_among_them(pref):
    kept = [(p, c) + f for p, c, sample in P.PHOENIX_CYCLES for f in P.phoenix_cycles(pref, p, c, [(p, c, sample)])]
    assert [k[2] for k in kept] == [sample for _, _, sample in P.PHOENIX_CYCLES]
    for p, c, sample, found_z, found_state in kept:
        assert found_z % P.CHUNK == 0 and (found_state is None or (found_state % P.CHUNK == 0 and found_z < found_state))
    # the state found at 180: the second comparison after the first save, against the second save (at 120)
    assert any(fs == 180 for *_, fs in kept)
    # the state found after a later save, z found no later than that save is made ... and strictly before it
    later = [(fz, fs) for *_, fz, fs in kept if fs is not None and fs >= 240]
    assert any(fz <= P.last_save_before(fs) for fz, fs in later) and any(fz < P.last_save_before(fs) for fz, fs in later)
    assert any(fs is None for *_, fs in kept)  # and one that z alone would retire and the state never does


def test_the_search_finds_the_searched_candidates_again(pref):
    """phoenix_cycle_search is where a replacement comes from: it names both searched candidates with the chunks the
    restatement confirms, and every kind of plant the floor asks for is among what it finds."""
    p, c = (-0.5, 0.0), None
    hits = P.phoenix_cycle_search(p[0])
    for sample in ((-1.80267333984375, 0.0), (-1.4501953125, 0.0)):
        assert (p, c, sample) in P.PHOENIX_CYCLES
        ((_, found_z, found_state),) = P.phoenix_cycles(pref, p, c, [(p, c, sample)])
        assert sample[0] in hits[found_z, found_state]
    assert hits[180, 240] and hits[180, 360] and hits[180, None]
    for key in ((180, 240), (180, 360), (180, None)):  # the first hit of each kind is confirmed as that kind
        sample = (hits[key][0], 0.0)
        assert P.phoenix_cycles(pref, p, c, [(p, c, sample)]) == [(sample,) + key]


@pytest.mark.parametrize("case", range(len(P.PHOENIX_CYCLES)), ids=lambda k: "%d" % k)
def test_the_two_discounts_of_a_cycle_plant(pref, case):
    p, c, sample = P.PHOENIX_CYCLES[case]
    ((_, found_z, found_state),) = P.phoenix_cycles(pref, p, c, [(p, c, sample)])
    for max_iter in P.cycle_max_iters(found_z, found_state):
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            extra = {}
            _, wc = draw(pref, points, max_iter, 1, p, c, extra=extra)
            assert wc["never_escaped"] == n and wc["too_fast"] == 64 - n and wc["recorded"] == 0
            assert extra["skipped_z_only"] == n * P.cycle_discount(found_z, max_iter)
            assert extra["skipped_state"] == n * P.cycle_discount(found_state, max_iter)
            assert (extra["skipped_z_only"] != extra["skipped_state"]) == (max_iter > found_z)
            assert extra["cycles_z_only"] == (n if max_iter > found_z else 0)
            assert extra["cycles_state"] == (n if found_state is not None and max_iter > found_state else 0)


def test_two_plants_lane_by_lane_discount_the_sum(pref):
    (p, c, a), (_, _, b) = P.PHOENIX_CYCLES[0], P.PHOENIX_CYCLES[1]
    assert (p, c) == P.PHOENIX_CYCLES[1][:2]
    ((_, _, state_a),) = P.phoenix_cycles(pref, p, c, [(p, c, a)])
    ((_, _, state_b),) = P.phoenix_cycles(pref, p, c, [(p, c, b)])
    assert state_a != state_b
    extra = {}
    draw(pref, P.cycled([a, b], 64), 300, 1, p, c, extra=extra)
    assert extra["skipped_state"] == 32 * (300 - state_a) + 32 * (300 - state_b)


# ---- 3. the circle ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(P.PHOENIX_CIRCLE))
def test_circle_plants_are_on_the_circle_exactly(pref, name):
    p, c, sample, on_circle, end = P.PHOENIX_CIRCLE[name]
    cr, ci = sample if c is None else c
    state, norms = (sample[0], sample[1], 0.0, 0.0), []
    for _ in range(40):
        *state, m = phoenix.step(pref, cr, ci, p[0], p[1], *state)
        norms.append(m)
    assert all(norms[k - 1] == 4.0 for k in on_circle)
    assert end_by_hand(pref, sample, p, c, 121) == end
    if name == "sampled":
        assert norms[1] == 4.5 * 4.5  # z_2 = 4.5
        for max_iter in (2, 3, 121):
            _, wc = draw(pref, P.lanes(sample), max_iter, 1, p, c, box=P.WIDE_BOX)
            assert wc["recorded"] == 1 and wc["replay_steps"] == 2 and wc["increments"] == 1  # z_1 = 2 is on WIDE_BOX, 4.5 is not
        _, wc = draw(pref, P.lanes(sample), 1, 0, p, c)  # max_iter 1: z_1 does not escape, a >= would record it
        assert wc["never_escaped"] == 1
    else:
        assert max(norms) == 4.0
        for max_iter in (3, 4, 121):
            _, wc = draw(pref, P.lanes(sample), max_iter, 1, p, c, box=P.WIDE_BOX)
            assert wc["never_escaped"] == 1 and wc["recorded"] == 0


# ---- 4. the replay plant ---------------------------------------------------------------------------------------------------------


def test_the_replay_plants_points_are_the_restatements(pref, ref):
    r = P.PHOENIX_REPLAY
    points, end = P.orbit_of(pref, r["sample"], 5, phoenix=r["p"])
    assert end == r["end"] and points == r["points"]
    hist, wc = draw(pref, P.lanes(r["sample"]), 2, 1, r["p"], box=P.WIDE_BOX)
    want = P.histogram(P.WIDE_BOX, W, H, *zip(*points))
    assert wc["recorded"] == 1 and wc["increments"] == 2 and np.array_equal(hist, want)
    # what a replay that began with ITERATE's y (z_1) would plot first: one step from (z_0, y = z_1), another pixel
    z_0, z_1 = r["sample"], points[0]
    wrong = phoenix.step(pref, *z_0, *r["p"], *z_0, *z_1)[:2]
    assert wrong == r["wrong_first"]
    assert not np.array_equal(P.histogram(P.WIDE_BOX, W, H, [wrong[0]], [wrong[1]]), P.histogram(P.WIDE_BOX, W, H, [z_1[0]], [z_1[1]]))
    # under another projection: projected_orbit's points on phoenix.step, plotted by plot.point, are the restatement's
    u, v, end = P.projected_orbit(pref, plot.HOLOGRAM, r["sample"], 5, plot_lib=ref, phoenix=r["p"])
    hist, wc = phoenix.draw(pref, W, H, 2, 1, 64, [1], p=r["p"], projection=plot.HOLOGRAM, box=P.WIDE_BOX,
                            states=P.plant_states(P.lanes(r["sample"])))
    assert end == 2 and wc["increments"] == 2 and np.array_equal(hist, P.histogram(P.WIDE_BOX, W, H, u, v))
    assert not np.array_equal(hist, want)
    # and a longer one, found: 13 points, all but the escaping one on the canvas
    p, c = P.PHOENIX_SETTINGS["sampled"]
    sample = P.with_end(pref, 13, c, phoenix=p)
    points, end = P.orbit_of(pref, sample, 13, phoenix=p)
    hist, wc = draw(pref, P.lanes(sample), 13, 1, p, box=P.WIDE_BOX)
    assert end == 13 and np.array_equal(hist, P.histogram(P.WIDE_BOX, W, H, *zip(*points))) and wc["increments"] >= 12


# ---- 5. p = 0 --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [None, P.FIXED_C], ids=["sampled", "fixed"])
def test_p_zero_is_the_mandelbrot_step_without_rejection_on_planted_states(pref, ref, c):
    samples = [P.with_end(ref, end, c) for end in P.ENDS]
    for end, sample in zip(P.ENDS, samples):
        assert end_by_hand(pref, sample, (0.0, 0.0), c, 200) == end
    points = P.cycled(samples, 512)
    a, b = P.plant_states(points), P.plant_states(points)
    hist, wc = phoenix.draw(pref, W, H, 121, 12, 512, [1, 50], p=(0.0, 0.0), c=c, states=a)
    want, pc = plot.draw(ref, W, H, 121, 12, 512, [1, 50], c=c, reject=False, states=b)
    assert wc == pc and np.array_equal(hist, want) and np.array_equal(a, b) and wc["recorded"] > 512 * 4 // 7


# ---- 6. negative zeros -----------------------------------------------------------------------------------------------------------


def test_the_negative_zero_plants(pref):
    signs = {}
    for name, (p, c, sample) in P.PHOENIX_ZEROS.items():
        state, seen = (sample[0], sample[1], 0.0, 0.0), []
        for _ in range(24):
            *state, m = phoenix.step(pref, c[0], c[1], p[0], p[1], *state)
            seen.append(tuple(state))
        signs[name] = [np.signbit(s[1]) for s in seen]
        assert all(s[1] == 0.0 for s in seen)
        if name == "p_zero":  # 0 -> -1 -> 0 in value, period 4 in the sign of the zero
            assert [s[0] for s in seen] == [-1.0, 0.0] * 12
            assert signs[name] == [False, True, False, False] * 6
            assert [np.array(s).tobytes() for s in seen[4:]] == [np.array(s).tobytes() for s in seen[:-4]]
            assert np.array(seen[2]).tobytes() != np.array(seen[0]).tobytes()
        ((_, found_z, found_state),) = P.phoenix_cycles(pref, p, c, [(p, c, sample)])
        assert found_z == found_state
        for max_iter in P.ZEROS_MAX_ITERS:
            extra = {}
            _, wc = draw(pref, P.lanes(sample, shape="all64"), max_iter, 1, p, c, extra=extra)
            assert wc["never_escaped"] == 64 and extra["skipped_state"] == 64 * P.cycle_discount(found_state, max_iter)
    assert any(signs["p_half"])  # it does pass a negative zero
