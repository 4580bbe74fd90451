"""The planted arrays of tests/output_planted.py are decisive: shown here on the host functions alone (cb_tone_value
through cb.set_grayscale_pixels, cb_compose_color, tests/color_reference.py), so that the GPU suites which feed them
to tonemap.hip and color.hip test what they say they test."""

import numpy as np
import pytest

import color_reference as ref
import output_planted as op


# ---- tone map ----


@pytest.mark.parametrize("top", op.DOMAIN_TOPS)
def test_every_count_of_a_domain_is_planted_once(top):
    a = op.every_count(top)
    assert a.dtype == np.uint64 and np.array_equal(np.sort(a), np.arange(top + 1, dtype=np.uint64))
    assert top < 100 or not np.array_equal(a, np.sort(a))  # shuffled


def test_a_brightest_value_below_65535_exists(cb):
    """For a maximum of 162 at gamma 1.0 the host's brightest value is 65534: 162 * (65535.0 / 162) rounds below 65535
    and the conversion truncates.  The last threshold of the device's table then has no count."""
    assert cb.tone_value(162, 162, 1.0) == 65534
    gray, mx, _ = cb.set_grayscale_pixels(op.every_count(162).reshape(1, -1), 1.0)
    assert mx == 162 and int(gray.max()) == 65534
    assert cb.tone_value(65535, 65535, 1.0) == 65535  # and the usual case is among the domains too


@pytest.mark.parametrize("gamma", op.GAMMAS)
@pytest.mark.parametrize("top", op.BEYOND_TOPS)
def test_threshold_plants_straddle_every_step_of_the_host_map(cb, top, gamma):
    value = op.host_map(cb, top, gamma)
    planted, edges = op.beyond_the_table(value, top)
    assert planted.size % 2 == 1 and int(planted.max()) == top
    present = set(planted.tolist())
    assert {0, 1, top - 1, top} <= present
    if top > 1 << 63:
        assert {(1 << 63) - 1, 1 << 63} <= present
    # every pair (t - 1, t) has two different host values, and there are as many pairs as distinct non-zero values: each
    # step of the map over the planted counts has its pair, exactly
    assert edges.min() >= 1 and np.all(value(edges - np.uint64(1)) != value(edges))
    assert {int(t) for t in edges} | {int(t) - 1 for t in edges} <= present
    values = np.unique(value(planted))
    assert edges.size == np.count_nonzero(values)
    assert edges.size > (60_000 if gamma != 2.2 else 30_000)  # nearly every output value is reached (a steep foot at 2.2)


@pytest.mark.parametrize("top", [1 << 40, (1 << 24) - 1])
def test_the_array_past_the_first_sweep_is_decided_behind_it(cb, top):
    value = op.host_map(cb, top, 2.2)
    a, edge = op.past_the_first_sweep(value, op.TONE_SWEEP, top)
    assert a.size == 2 * 4096 * 256 + 3 and a.size % 2 == 1
    assert a[-3:].tolist() == [0, edge, top] and int(a[:-3].max()) < 60_000
    assert np.count_nonzero(a == np.uint64(top)) == 1
    below, at = value([edge - 1, edge])
    assert below < at


def test_tiny_arrays():
    assert [op.tiny(n).tolist() for n in (1, 2, 3)] == [[5], [2, 5], [3, 2, 5]]


def test_the_clamp_instance_has_counters_above_its_white(cb):
    hist = op.every_count(1_000_003).reshape(1, -1)
    white, lit, clipped = cb.white_count(hist, 50.0)
    assert lit == 1_000_003 and 0 < white < 1_000_003 and clipped == 1_000_003 - white > 400_000


# ---- colour ----


def check_plant(cb, case):
    """The planes are their own tone map at gamma 0, and both host references find the designed levels."""
    planes, (b, w) = case["planes"], case["stretch"]
    n = planes[0].size
    assert (int(float(n) * (b / 100.0)), int(float(n) * (w / 100.0))) == case["ranks"] and b + w < 100.0
    grays = []
    for p in planes:
        gray, mx, scale = cb.set_grayscale_pixels(p, 0.0)
        assert mx == 65535 and scale == 1.0 and np.array_equal(gray, p)
        grays.append(gray)
    assert [ref.levels(g, b, w) for g in grays] == [tuple(lv) for lv in case["levels"]]
    assert cb.compose_color(grays, "rgb", (b, w))[1] == [tuple(lv) for lv in case["levels"]]
    return grays


@pytest.mark.parametrize("name", sorted(op.LEVEL_CASES))
def test_level_plants_have_the_designed_levels(cb, name):
    case = op.level_case(name)
    assert case["planes"][0].shape == (61, 67)
    grays = check_plant(cb, case)
    nb, nw = case["ranks"]
    for g, (black, white) in zip(grays, case["levels"]):
        s = np.sort(g.reshape(-1))
        assert (int(s[nb]), int(s[s.size - 1 - nw])) == (black, white)


def test_level_plants_cover_the_listed_rows(cb):
    cases = {name: op.level_case(name) for name in op.LEVEL_CASES}
    levels = [lv for c in cases.values() for lv in c["levels"]]
    assert (0x12ff, 0xa000) in levels                                      # last / first value of a bucket
    assert any(b >> 8 == w >> 8 and b < w for b, w in levels)              # one bucket
    assert any(b >> 8 == 0 and b & 255 and w >> 8 == 255 for b, w in levels)
    assert any(b == w for b, w in levels)                                  # white <= black
    assert all(b > 0 for b, w in levels[:-1]) and levels[-1][0] == 0      # a positive black everywhere but the last plane
    assert cases["zero_ranks"]["stretch"] == (0.0, 0.0)
    # the equalities: exactly nb pixels in lower buckets (coarse), exactly nb below black with some in its bucket (fine)
    c = cases["bucket_ends_and_equalities"]
    nb, nw = c["ranks"]
    for plane, coarse in ((c["planes"][1], True), (c["planes"][2], False)):
        black, white = 0x3105, 0xc2f0
        v = plane.reshape(-1).astype(np.int64)
        assert np.count_nonzero(v < black) == nb and np.count_nonzero(v > white) == nw
        assert (np.count_nonzero(v >> 8 < black >> 8) == nb) == coarse
        assert (np.count_nonzero(v >> 8 > white >> 8) == nw) == coarse
    # the ties: a rank either side of each level gives the same value
    t = np.sort(cases["one_bucket_extremes_ties"]["planes"][2].reshape(-1))
    nb, nw = cases["one_bucket_extremes_ties"]["ranks"]
    assert t[nb - 40] == t[nb + 40] == 0x4444 and t[t.size - 1 - nw - 40] == t[t.size - 1 - nw + 40] == 0x8888
    # no pixel below 1000
    assert int(cases["flat_bright_equality"]["planes"][1].min()) >= 1000 and cases["flat_bright_equality"]["levels"][1][0] > 0


def test_levels_past_the_sweep_are_the_tail_s(cb):
    case = op.levels_past_the_sweep(op.LEVEL_SWEEP)
    n = 1024 * 256 * 8 + 11
    assert all(p.shape == (1, n) for p in case["planes"]) and case["ranks"] == (5, 2)
    check_plant(cb, case)
    for p, (black, white) in zip(case["planes"], case["levels"]):
        head, tail = p[0, :-11], np.sort(p[0, -11:])
        assert np.all(head == 30_000) and np.unique(tail).size == 11 and 30_000 not in tail
        assert np.count_nonzero(tail < 30_000) == 7 and int(tail[-1]) == 65535
        assert (black, white) == (int(tail[5]), int(tail[-3])) and black < 30_000 < white < 65535


def test_compose_decisions_fall_on_both_sides(cb):
    case = op.compose_decisions()
    grays = check_plant(cb, case)
    triples = np.stack([g.reshape(-1) for g in grays], axis=1)
    assert np.unique(triples[:-3], axis=0).shape[0] == 16 ** 3 and triples.shape[0] == 4099
    s = [ref.stretch(g.reshape(-1), *op.DECISION_LEVELS) for g in grays]
    for x in s:
        assert x.min() == 0.0 and x.max() == 1.0 and np.count_nonzero(x == 0.0) and np.count_nonzero(x == 1.0)
    one = lambda v: float(ref.stretch(np.array([v], dtype=np.uint16), *op.DECISION_LEVELS)[0])  # noqa: E731
    assert one(35534) < 0.5 <= one(35536) and one(35535) == 0.5              # L < 0.5, from both sides and on it
    L = s[2]
    assert np.any(L < 0.5) and np.any(L >= 0.5)
    for _, shift in op.COMPOSES[1:]:
        h = s[0] + shift
        h = h - np.floor(h)
        t = np.concatenate([h + 1.0 / 3.0, h, h - 1.0 / 3.0])               # the three channels of color_compose
        t = t - np.floor(t)
        for edge in (1.0 / 6.0, 0.5, 2.0 / 3.0):                            # color_hsl_channel's comparisons, in its order
            assert np.any(t < edge) and np.any(t >= edge), (shift, edge)
            t = t[t >= edge]
    # and with no shift the planted neighbours lie on either side of each edge
    for v, edge in ((15535, 1.0 / 6.0), (35535, 0.5), (45535, 2.0 / 3.0)):
        assert one(v - 1) < edge < one(v + 1)
