"""The period-palette render's kernels at the edges of their schedule, modelled on tests/test_gpu_bounded_edges.py: the
product kernel (28), the lock-step kernel (29) and the restatement (tests/period_reference.c), three ways, where

  M   is at a round's edge (11, 12, 13), at a chunk's (59, 60, 61), below, at and above the first comparison a sample can
      pass (119, 120 -- a cycle found AT k == M, rem == 0: the probe is z_s itself --, 121: the probe is one step on), and
      at the second (180, 181); M <= 0 is the kernels' early path;
  J   is 1 and 2, at a round's edge of the search (11, 12, 13 steps are inside a longer search; 59, 60, 61 end one), and the
      largest, 1023;
  the grid is 1, 63, 64, 65 and 257 threads: less than a wave, a whole one, one lane more, a ragged second workgroup;
  the launches are of one sample;
  the canvas is one nothing reaches;
  the table is all zero (nothing is replayed, the planes stay zero), or zero at entry 0 only;
  eps is 0x1p+10: every bounded sample of the reference's step has period 1;

each with a sampled and a fixed c.  The restatement's `extra` shows that an input reaches the branch it is meant to reach."""

import numpy as np
import pytest

import period_reference as period
from period_harness import pref, three_ways  # noqa: F401

pytestmark = pytest.mark.gpu

CROP = (-1.5, 0.7, -0.9, 1.1)
SOURCES = {"sampled": None, "fixed": (-1.0, 0.0)}
EDGE_M = [-3, 0, 1, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 181]
EDGE_J = [1, 2, 59, 60, 61, 1023]
SMALL = dict(threads=257, launches=(3, 20, 1), box=CROP)
CYCLES = ("cycle_period", "cycle_none")


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("max_iter", EDGE_M)
def test_max_iterations_at_the_schedules_edges(cb, pref, oracle, max_iter, source):  # noqa: F811
    lut = period.gradient_table(8)
    lut[3] = 0
    want, wc, extra, product = three_ways(cb, pref, oracle, lut, max_iter=max_iter, c=SOURCES[source], **SMALL)
    cycles = sum(extra[k] for k in CYCLES)
    assert wc["recorded"] > 0
    if max_iter <= 0:  # nothing is tested and nothing is added; the search runs from z_0 and is counted nowhere
        assert wc["recorded"] == wc["samples"] and wc["iterate_steps"] == 0 and wc["replay_steps"] == 0
        assert wc["increments"] == 0 and not want.any() and product["skipped_steps"] == 0
        return
    assert extra["escaped"] > 0 and wc["increments"] > 0
    if max_iter < 120:  # a point is first saved at 60 and first matched at 120
        assert cycles == 0 and product["skipped_steps"] == max_iter * extra["zero_entry"]
    else:
        assert cycles > 0
    if max_iter in (120, 180):  # every cycle is found with remainder 0
        assert extra["rem_zero"] == cycles
    if max_iter in (121, 181):
        assert extra["rem_zero"] == 0 and product["skipped_steps"] > 0


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("j", EDGE_J)
def test_table_lengths_at_the_searchs_edges(cb, pref, oracle, j, source):  # noqa: F811
    # M = 130: orbits without an exact cycle search all J steps; M = 181: exact cycles walk rem = 1 step first
    for max_iter in (130, 181):
        _, wc, extra, product = three_ways(cb, pref, oracle, period.gradient_table(j + 1), max_iter=max_iter,
                                           c=SOURCES[source], **SMALL)
        assert wc["recorded"] > 0 and wc["increments"] > 0
        if source == "sampled":
            assert extra["tol_none"] > 0  # a search that runs to its end
        if j == 1 and max_iter == 181:
            assert extra["cycle_none"] > 0  # the period-2 cycles


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("threads", [1, 63, 64, 65, 257])
def test_grids_below_at_and_above_a_wave(cb, pref, oracle, threads, source):  # noqa: F811
    launches = (400,) if threads == 1 else (3, 20, 1)
    _, wc, extra, product = three_ways(cb, pref, oracle, period.gradient_table(256), max_iter=181, threads=threads,
                                       launches=launches, box=CROP, c=SOURCES[source])
    assert wc["recorded"] > 0 and extra["escaped"] > 0 and extra["cycle_period"] > 0 and product["skipped_steps"] > 0


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("launches", [(1,), (1, 1, 1)], ids=["one", "three_of_one"])
def test_launches_of_one_sample(cb, pref, oracle, launches, source):  # noqa: F811
    _, wc, extra, _ = three_ways(cb, pref, oracle, period.gradient_table(256), max_iter=181, threads=1000, launches=launches,
                                 box=CROP, c=SOURCES[source])
    assert wc["samples"] == 1000 * len(launches) and wc["recorded"] > 0 and extra["cycle_period"] > 0


def test_a_canvas_nothing_reaches(cb, pref, oracle):  # noqa: F811
    want, wc, extra, product = three_ways(cb, pref, oracle, period.gradient_table(256), box=(10.0, 11.0, 10.0, 11.0),
                                          launches=(20,))
    assert wc["recorded"] > 0 and wc["replay_steps"] > 0 and wc["increments"] == 0 and not want.any()
    assert product["skipped_steps"] > 0


@pytest.mark.parametrize("source", list(SOURCES))
def test_an_all_zero_table_replays_nothing(cb, pref, oracle, source):  # noqa: F811
    lut = np.zeros(256, dtype=np.uint32)
    want, wc, extra, product = three_ways(cb, pref, oracle, lut, launches=(20,), box=CROP, c=SOURCES[source])
    assert wc["recorded"] == extra["zero_entry"] > 0 and wc["replay_steps"] == 500 * wc["recorded"]
    assert wc["increments"] == 0 and not want.any()
    # every replay is booked as not made, beside the iteration's own discount
    assert product["skipped_steps"] >= wc["replay_steps"]


@pytest.mark.parametrize("source", list(SOURCES))
def test_a_table_that_is_zero_at_entry_zero_only(cb, pref, oracle, source):  # noqa: F811
    lut = period.gradient_table(256)
    lut[0] = 0
    # M = 130: a sampled c has orbits without a period; the basilica's all have period 2
    want, wc, extra, product = three_ways(cb, pref, oracle, lut, max_iter=130, launches=(20,), box=CROP, c=SOURCES[source])
    none = extra["cycle_none"] + extra["tol_none"]
    assert extra["zero_entry"] == none and wc["increments"] > 0
    assert (none > 0) == (source == "sampled")


@pytest.mark.parametrize("j", [1, 255])
def test_a_wide_eps_gives_every_bounded_sample_period_one(cb, pref, oracle, j):  # noqa: F811
    want, wc, extra, product = three_ways(cb, pref, oracle, period.one_hot(j + 1, 1, 0x020301), 2.0 ** 10, launches=(20,),
                                          box=CROP)
    assert extra["zero_entry"] == extra["cycle_none"] == extra["tol_none"] == 0 and wc["recorded"] > 0
    assert extra["search_steps"] == wc["recorded"]  # one step each
    assert np.array_equal(want[0], want[2] // 2) and np.array_equal(want[1], 3 * want[0]) and want[0].any()
