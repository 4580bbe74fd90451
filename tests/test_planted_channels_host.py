"""The fused render's planted cases (tests/planted_samples.py, "the cases both channel suites use") on the oracle alone,
before a kernel sees them: every window edge of every set of CHANNEL_SETS has a planted count either side of it that the
oracle's render of that window tells apart; fused_model -- the restatement of DESIGN.md 4.6 that the GPU suite holds the
kernel's counters to -- agrees with the oracle's separate renders wherever the oracle has a say; and every set has the
orbits it is named for: direct and measured ones, orbits in one, two and four planes, the three fates in balance.
tests/test_gpu_planted_channels.py gives the same inputs to cb_draw_buddhabrot_channels; what it can catch is what is
shown here.  The conditions are conditions on the INPUTS: a set that fails one is changed, not the condition."""

import numpy as np
import pytest

import planted_samples as P
from device_launches import SQUARE

THREADS = 512
W, H = 96, 80
SETS = sorted(P.CHANNEL_SETS)
edge_inside_min, edge_inside_max = (0, 1), (1, 0)      # `recorded` of (edge - 1, edge) at a window's min and at its max


def render(oracle, points, window, samples=1):
    """One oracle run of the window over the planted states -> (hist, counters)."""
    return oracle.render(W, H, window[0], window[1], len(points), 1, SQUARE, samples_per_thread=samples,
                         states=P.plant_states(points))


@pytest.fixture(scope="module")
def planted():
    """Per set: (samples, points of the layout, their counts, the model of the layout)."""
    out = {}
    for name, windows in P.CHANNEL_SETS.items():
        samples, points = P.channel_layout(windows, THREADS)
        counts = P.counts_of(points, P.hull(windows)[0] + 2)
        out[name] = (samples, points, counts, P.fused_model(windows, counts))
    return out


def test_the_hull_and_the_stage_plan_are_what_the_sets_are_named_for():
    """The arithmetic the table of sets rests on: hulls, long_start 20 (40 for the deep min), no tail chunk, a tail chunk
    of 1 step and of 59, a hull inside HEAD + MID."""
    S = P.CHANNEL_SETS
    assert P.hull(S["recipe_deepest_first"]) == (60000, 20) and P.hull(S["empty_windows_among_others"]) == (500, 50)
    assert P.hull(S["nested_four"]) == (3000, 20) and P.hull(S["shallow"]) == (16, 0)
    assert P.stage_plan(*P.hull(S["edges_on_chunk_starts"])) == (20, 2540)              # tail_start == max: no tail chunk
    assert P.stage_plan(*P.hull(S["edges_one_past_a_start"])) == (20, 2540)             # [2540, 2541)
    assert P.stage_plan(*P.hull(S["edges_on_a_chunk_s_last_index"])) == (20, 2540)      # [2540, 2599)
    assert P.stage_plan(*P.hull(S["hull_min_deep"])) == (40, 2980) and (1000 - 40) % P.CHUNK == 0
    assert P.stage_plan(*P.hull(S["shallow"])) == (None, None)
    assert P.stage_plan(1234, 20) == (20, 1220) and P.stage_plan(3000, 1000) == (40, 2980)   # the earlier callers' values
    for m, c in S["edges_on_chunk_starts"]:
        assert (m - 20) % P.CHUNK == 0 == (c - 20) % P.CHUNK
    assert P.chunk_of(141, 20) == (140, 199) == P.chunk_of(199, 20) and P.chunk_of(1007, 40) == (1000, 1059)
    assert all(len(w) <= 4 for w in S.values())


@pytest.mark.parametrize("name", SETS)
def test_every_edge_has_a_planted_count_either_side_that_the_oracle_tells_apart(oracle, name):
    """For every window with indices in it and each of its two edges e: e - 1 and e are planted (from count 1 on: nothing
    below a min of 0 or 1 can be), and the oracle's render of that window alone on the one and on the other gives
    different planes -- one orbit recorded, or none.  An empty window's plane is zero on all planted samples."""
    windows = P.CHANNEL_SETS[name]
    samples = P.channel_samples(windows)
    by_count = {}
    for n, c in samples:
        assert P.escape_count(*c, P.hull(windows)[0] + 5) == n and not P.rejected(*c)
        by_count.setdefault(n, []).append(c)
    assert all(len(v) == 2 and v[0] != v[1] for v in by_count.values())       # both rays
    top, low = P.hull(windows)
    assert {top - 1, top, top + 1} <= set(by_count)
    for window in dict.fromkeys(windows):
        m, c = window
        if c >= m:
            hist, cnt = render(oracle, [p for _, p in samples], window)
            assert not hist.any() and cnt["recorded"] == 0
            continue
        for edge, inside in ((c, edge_inside_min), (m, edge_inside_max)):
            if edge < 2:
                continue
            for ray in (0, 1):
                below, cb_ = render(oracle, [by_count[edge - 1][ray]], window)
                above, ca = render(oracle, [by_count[edge][ray]], window)
                assert not np.array_equal(below, above), (name, window, edge)
                assert (cb_["recorded"], ca["recorded"]) == inside, (name, window, edge)


@pytest.mark.parametrize("name", SETS)
def test_the_model_agrees_with_the_oracle(oracle, planted, name):
    """On the layout the GPU suite launches: the model's orbits per plane are the oracle's `recorded` of that window, its
    rejected and never_escaped those of the hull window, its `recorded` what recorded_by_windows makes of the oracle's
    separate runs, and its replay_steps lie between the per-window sum and that plus the hull's -- the lower bound is met
    exactly where nothing is measured.  The oracle has no word on direct or measured: those are the next test's."""
    windows = P.CHANNEL_SETS[name]
    samples, points, counts, model = planted[name]
    singles = [render(oracle, points, w)[1] for w in windows]
    of_hull = render(oracle, points, P.hull(windows))[1]
    assert model["planes"] == [s["recorded"] for s in singles]
    assert model["rejected"] == of_hull["rejected"] == 0 and model["never_escaped"] == of_hull["never_escaped"]
    assert model["recorded"] == P.recorded_by_windows(windows, [s["recorded"] for s in singles], of_hull["recorded"])
    assert model["recorded"] + model["too_fast"] == THREADS - of_hull["rejected"] - of_hull["never_escaped"]
    low = sum(s["replay_steps"] for s in singles)
    assert low <= model["replay_steps"] <= low + of_hull["replay_steps"]
    measured = sum(k + 1 for k, (_, how) in zip(counts, model["samples"]) if how == "measured")
    assert model["replay_steps"] == low + measured


def test_nested_four_has_orbits_in_one_two_and_four_planes(planted):
    _, _, _, model = planted["nested_four"]
    assert {len(planes) for planes, how in model["samples"] if how} == {1, 2, 4}
    assert all(len(planes) != 3 for planes, _ in model["samples"])


@pytest.mark.parametrize("name", SETS)
def test_direct_and_measured_orbits_of_the_long_stage(planted, name):
    """Every set with a LONG stage has, among its planted samples, an orbit that escapes in a full LONG chunk and is
    direct and one that is measured -- but edges_on_chunk_starts, where no planted orbit at all is measured.  The sets
    without a LONG stage or with a min inside HEAD / MID have measured orbits that no chunk is known of."""
    windows = P.CHANNEL_SETS[name]
    samples, points, counts, model = planted[name]
    long_start, tail_start = P.stage_plan(*P.hull(windows))
    hows = [how for _, how in model["samples"]]
    if name == "edges_on_chunk_starts":
        assert "measured" not in hows and hows.count("direct") >= THREADS // 8
        return
    if long_start is None:
        assert "direct" not in hows and "measured" in hows
        return
    in_long = {how for k, how in zip(counts, hows) if how and long_start <= k < tail_start}
    assert in_long == {"direct", "measured"}, (name, in_long)
    in_tail = {how for k, how in zip(counts, hows) if how and k >= tail_start}
    assert in_tail <= {"measured"} and (in_tail or tail_start == P.hull(windows)[0])
    before = {how for k, how in zip(counts, hows) if how and k < long_start}
    assert before <= {"measured"}
    if name == "gap_min_below_head":
        assert before == {"measured"}
    if name in ("recipe_deepest_first", "gap_min_below_head"):     # in a gap: accepted, measured, in no plane
        assert any(how == "measured" and not planes for planes, how in model["samples"])


@pytest.mark.parametrize("name", SETS)
def test_the_three_fates_each_get_an_eighth_of_the_lanes(planted, name):
    """Wherever the set admits all three.  `shallow` has a min of 0 and no gap: nothing escapes too fast there."""
    windows = P.CHANNEL_SETS[name]
    samples, points, counts, model = planted[name]
    assert len(points) == THREADS and {c for _, c in samples} <= set(points)
    single = P.fused_model(windows, [n for n, _ in samples])
    admits = [k for k in ("recorded", "too_fast", "never_escaped") if single[k]]
    assert admits == ["recorded", "too_fast", "never_escaped"] or name == "shallow"
    assert min(model[k] for k in admits) >= THREADS // 8, {k: model[k] for k in admits}


@pytest.mark.parametrize("name", ["nested_four", "edges_one_past_a_start"])
def test_the_occupancy_counts_cover_every_kind_of_orbit(name):
    """What the sparse layouts of the GPU suite plant: every (planes, direct | measured) the set's counts have, and an
    orbit that never escapes."""
    windows = P.CHANNEL_SETS[name]
    counts = P.occupancy_counts(windows)
    kinds = {s for s in P.fused_model(windows, counts)["samples"] if s[1]}
    assert kinds == {s for s in P.fused_model(windows, P.channel_counts(windows))["samples"] if s[1]}
    assert P.hull(windows)[0] in counts and 4 <= len(counts) <= 16
    assert {how for _, how in kinds} == {"direct", "measured"}
