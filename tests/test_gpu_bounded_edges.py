"""The bounded render's kernels at the edges of their schedule, modelled on tests/test_gpu_anti_edges.py: the product
kernel (26), the lock-step kernel (27) and the restatement (tests/bounded_reference.c), three ways, where

  M   is at a round's edge (11, 12, 13), at a chunk's (59, 60, 61), below, at and above the first comparison a sample can
      pass (119, 120 -- a cycle found AT k == M, (M - s) % p == 0 --, 121), and at the second (180, 181: the weight split
      q + 1 / q with remainder 0 and 1); M <= 0 is the kernels' early path;
  the launches are of one sample;
  the grid is 1, 63, 64, 65 and 257 threads: less than a wave, a whole one, one lane more, a ragged second workgroup;

each with a sampled and a fixed c.  The restatement's `extra` shows that an M reaches the branch it is meant to reach."""

import pytest

from bounded_harness import bref, three_ways  # noqa: F401

pytestmark = pytest.mark.gpu

CROP = (-1.5, 0.7, -0.9, 1.1)
SOURCES = {"sampled": None, "fixed": (-1.0, 0.0)}
EDGE_M = [0, 1, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 181]


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("max_iter", EDGE_M + [-3])
def test_max_iterations_at_the_schedules_edges(cb, bref, oracle, max_iter, source):  # noqa: F811
    want, wc, extra, product = three_ways(cb, bref, oracle, max_iter=max_iter, threads=257, launches=(3, 20, 1), box=CROP,
                                          c=SOURCES[source])
    assert wc["recorded"] > 0
    if max_iter <= 0:  # nothing is tested and nothing is added
        assert wc["recorded"] == wc["samples"] and wc["iterate_steps"] == 0 and wc["replay_steps"] == 0
        assert wc["increments"] == 0 and not want.any() and product["skipped_steps"] == 0
        return
    assert extra["escaped"] > 0 and wc["increments"] > 0
    if max_iter < 120:  # a point is first saved at 60 and first matched at 120
        assert extra["cycles"] == 0 and product["skipped_steps"] == 0
    else:
        assert extra["cycles"] > 0
    if max_iter == 120:  # s = 60, p = 60: found at k == M; z_60 twice in the place of z_120: one step saved per cycle
        assert extra["at_m"] == extra["rem_zero"] == extra["cycles"] == product["skipped_steps"]
    if max_iter == 121:
        assert extra["rem_zero"] == 0 and extra["both_weights"] == extra["cycles"] and product["skipped_steps"] > 0
    if max_iter == 180:  # p = 60 and s = 60 (found at 120) or s = 120 (found at k == M): rem = 0 either way
        assert extra["rem_zero"] == extra["cycles"] > extra["at_m"] and product["skipped_steps"] > 0
    if max_iter == 181:
        assert extra["rem_zero"] == 0 and product["skipped_steps"] > 0


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("threads", [1, 63, 64, 65, 257])
def test_grids_below_at_and_above_a_wave(cb, bref, oracle, threads, source):  # noqa: F811
    launches = (400,) if threads == 1 else (3, 20, 1)
    _, wc, extra, product = three_ways(cb, bref, oracle, max_iter=181, threads=threads, launches=launches, box=CROP,
                                       c=SOURCES[source])
    assert wc["recorded"] > 0 and extra["escaped"] > 0 and extra["cycles"] > 0 and product["skipped_steps"] > 0


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("launches", [(1,), (1, 1, 1)], ids=["one", "three_of_one"])
def test_launches_of_one_sample(cb, bref, oracle, launches, source):  # noqa: F811
    _, wc, extra, _ = three_ways(cb, bref, oracle, max_iter=181, threads=1000, launches=launches, box=CROP, c=SOURCES[source])
    assert wc["samples"] == 1000 * len(launches) and wc["recorded"] > 0 and extra["cycles"] > 0


def test_a_canvas_nothing_reaches(cb, bref, oracle):  # noqa: F811
    want, wc, extra, product = three_ways(cb, bref, oracle, box=(10.0, 11.0, 10.0, 11.0), launches=(20,))
    assert wc["recorded"] > 0 and wc["replay_steps"] > 0 and wc["increments"] == 0 and not want.any()
    assert extra["in_canvas"] == 0 and product["skipped_steps"] > 0
