"""The frames render's point queue (draw_frames.hip, FramesMode::converged and ::drain) and the bounded render's
cycle-compressed weights (draw_plot.h, BoundedMode::never_escapes and ::point) on PLANTED samples (tests/planted_samples.py):
the lanes of a wave put in phase, so that the queue's fill before a drain is what the case says -- 64 at every hook, 126,
a remainder of 1 and of 63 at `last` --, and orbits that repeat bit for bit with period 1 and 2, so that the cycle found is
s = 60, p = 60 and rem = (max_iter - 60) % 60 takes the values 0, 1 and 59.  tests/test_planted_plot_host.py holds the model
of the queue that gives these fills, and why 126 is the largest there is with one sample per subsequence.

Frames: product kernel (22) == lock-step kernel (23) == tests/frames_reference.py, bit for bit on the F planes, the counters
of SAME, the generator states and status 0.  Bounded: bounded_harness.three_ways, product (26) == lock-step (27) ==
tests/bounded_reference.c, skipped_steps included."""

import numpy as np
import pytest

import bounded_harness
import frames_reference as frames
import planted_samples as P
import plot_reference as plot
from bounded_harness import bref  # noqa: F401
from plot_harness import SAME, SQUARE, omp_threads, planar_states, ref, variant_of  # noqa: F401
from test_gpu_frames import LOCKSTEP, PRODUCT, frames_launches

pytestmark = pytest.mark.gpu

W, H = 64, 48
THREE = [plot.IDENTITY, plot.C_PLANE, plot.HOLOGRAM]
IDLE = (0.0, 0.0)          # rejected under the Mandelbrot step on a sampled c: idle whatever min_iter is
STAYS = (0.5, 0.0)         # under the fixed c = 1/4 the fixed point: it never escapes and notes nothing


def eight(cb):
    return cb.frames_from_sweep(plot.HOLOGRAM, ("zi", "cr"), 0.0, 90.0, 8)[0]


def frames_three_ways(cb, ref, mats, points, max_iter, min_iter, launches=(1,), c=None, **step):
    """-> (the restatement's planes, its counters, the product's counters)."""
    before = P.plant_states(points)
    st = before.copy()
    want, wc = frames.draw(ref, mats, W, H, max_iter, min_iter, len(points), list(launches), states=st, c=c,
                           omp_threads=omp_threads(), **step)
    got = {}
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, states = frames_launches(cb, variant_of(cb, base, **step), mats, c, w=W, h=H, max_iter=max_iter,
                                                      min_iter=min_iter, threads=len(points), launches=launches, states=before)
        assert launched == kernel and cnt["status"] == 0
        assert {k: cnt[k] for k in SAME} == wc, (kernel, cnt, wc)
        assert hist.shape == want.shape and np.array_equal(hist, want), kernel
        assert np.array_equal(states, planar_states(st)), kernel
        got[kernel] = cnt
    assert got[LOCKSTEP]["skipped_steps"] == 0
    return want, wc, got[PRODUCT]


def wave(sample, n, idle):
    return [sample] * n + [idle] * (64 - n)


# (lanes planted, end, min_iter, the queue: fills before a drain, remainder at `last`)
QUEUES = {
    "64_in_phase": (64, 13, 1, [64] * 13, 0),
    "64_in_phase_past_a_chunk": (64, 61, 1, [64] * 61, 0),
    "63_and_a_filler_reach_126": (63, 13, 1, list(range(126, 114, -1)), 51),
    "one_point_orbit": (1, 1, 0, [], 1),
    "63_one_point_orbits": (63, 1, 0, [], 63),
}


@pytest.mark.parametrize("c", [None, P.FIXED_C], ids=["sampled", "fixed"])
@pytest.mark.parametrize("name", list(QUEUES))
def test_the_queue_at_the_fills_the_case_names(cb, ref, name, c):
    n, end, min_iter, fills, rest = QUEUES[name]
    idle = P.FILLER if min_iter else (IDLE if c is None else STAYS)
    assert P.queue_fills([end] * n + [None] * (64 - n), min_iter) == (fills, rest)
    points = wave(P.with_end(ref, end, c), n, idle)
    for mats in (THREE, eight(cb)):
        want, wc, product = frames_three_ways(cb, ref, mats, points, max(end, 2), min_iter, c=c)
        assert product["recorded"] == n and product["replay_steps"] == n * end == 64 * len(fills) + rest
        if c is None:  # the C_PLANE frame: every point of every orbit in c's pixel
            assert mats is not THREE or int(want[1].max()) == n * end == int(want[1].sum())


@pytest.mark.parametrize("c", [None, P.FIXED_C], ids=["sampled", "fixed"])
def test_four_waves_queues_side_by_side_in_two_blocks(cb, ref, c):
    """512 subsequences: eight waves, each with a fill of its own (64 in phase at two ends, 63 and a filler, one lane, ends
    mixed), so that a wave that read or wrote its neighbour's queue would show; then 50 samples of the generators' own."""
    ends = [P.with_end(ref, e, c) for e in (13, 61, 12, 25, 2)]
    points = (wave(ends[0], 64, P.FILLER) + wave(ends[1], 64, P.FILLER) + wave(ends[0], 63, P.FILLER) + wave(ends[4], 63, P.FILLER)
              + wave(ends[2], 1, P.FILLER) + P.cycled(ends, 64) + wave(ends[3], 64, P.FILLER) + wave(ends[1], 32, P.FILLER))
    assert len(points) == 512
    for launches in ((1,), (1, 50)):
        want, wc, product = frames_three_ways(cb, ref, THREE, points, 121, 1, launches, c=c)
        assert all(p.any() for p in want)


def test_cardioid_and_bulb_neighbours_through_the_frames_kernel(cb, ref):
    pairs = P.cardioid_pairs(4) + P.bulb_pairs(4)
    points = P.cycled([p for pair in pairs for p in pair], 512)
    want, wc, product = frames_three_ways(cb, ref, THREE, points, 100, 20)
    assert product["rejected"] == sum(P.rejected(*p) for p in points) == 256


# ---- bounded ------------------------------------------------------------------------------------------------------------------

BOUNDED = P.REPEATING + [(P.MANDELBROT, None, (0.0, 0.0)), (P.MANDELBROT, None, (-1.0, 0.0))]  # nothing is rejected here


@pytest.mark.parametrize("max_iter", [120, 121, 179, 180, 181])
@pytest.mark.parametrize("case", range(len(BOUNDED)), ids=lambda k: "%d" % k)
def test_a_cycle_of_sixty_with_every_remainder(cb, ref, bref, oracle, case, max_iter):
    """The cycle is found at k = 120 against the point saved at 60: p = 60 whatever the least period (1 or 2), q =
    (max_iter - 60) / 60, rem = (max_iter - 60) % 60 = 0, 1, 59, 0, 1.  The lone orbit stays on the canvas: its increments are
    max_iter."""
    step, c, sample = BOUNDED[case]
    (found,) = [f for f in P.repeating(ref, step, c, BOUNDED) if f[0] == sample]
    for shape in ("lane0", "all64"):
        points = P.lanes(sample, 64, shape)
        n = points.count(sample)
        want, wc, extra, product = bounded_harness.three_ways(cb, bref, oracle, w=W, h=H, box=P.WIDE_BOX, max_iter=max_iter,
                                                              min_iter=0, threads=64, launches=(1,), c=c,
                                                              states=P.plant_states(points), **step)
        assert product["recorded"] == n and product["too_fast"] == 64 - n and product["increments"] == n * max_iter
        assert product["skipped_steps"] == n * ((max_iter - 120) + (max_iter - 119))
        assert 1 <= len(np.argwhere(want)) <= 2 and found[1] in (1, 2)
