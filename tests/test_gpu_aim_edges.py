"""The aimed render's kernels at their edges (draw_aim.hip), product (30) == lock-step (31) == restatement
(tests/aim_reference.c) bit for bit on mask, list, histogram, generator states and counters:

  the grid's two ends -- level 4 with no dilation, level 10 with a dilation of 2 on a 64 x 64 canvas -- with the model's
  figures for the issue's first window; a list of one entry and a list that is the whole grid; 1 .. 257 threads (one lane,
  a ragged wave, one past a workgroup); launches of one sample; a bounded M at and around the chunk boundaries of the
  cycle search (0, 1, 59, 60, 61, 120, 121); both sources of c.
"""

import numpy as np
import pytest

import aim_reference as aim
from aim_harness import BASES, aref, bits, gpu_draw, gpu_probe, same_counters, three_ways  # noqa: F401
from device_launches import SAME, omp_threads, planar_states

pytestmark = pytest.mark.gpu

FIRST = {k: v for k, v in aim.CASES["plane_zr_cr"].items() if k not in aim.MODEL_KEYS}
BOUNDED = {k: v for k, v in aim.CASES["bounded_zr_cr"].items() if k not in aim.MODEL_KEYS}
BOUNDED_JULIA = {k: v for k, v in aim.CASES["bounded_julia"].items() if k not in aim.MODEL_KEYS}
JULIA = {k: v for k, v in aim.CASES["julia"].items() if k not in aim.MODEL_KEYS}


def test_level_4_without_dilation(cb, aref, oracle):  # noqa: F811
    got = three_ways(cb, aref, oracle, **dict(FIRST, level=4, dilate=0))
    assert (bits(got["mask"]), len(got["cells"]), got["mask"].size * 32) == (8, 8, 4096)
    assert got["draw"][0]["increments"] > 0


def test_level_10_with_a_dilation_of_2(cb, aref, oracle):  # noqa: F811
    got = three_ways(cb, aref, oracle, **dict(FIRST, level=10, dilate=2, w=64, h=64, threads=4096, probe=(4,)))
    assert (bits(got["mask"]), len(got["cells"]), got["mask"].size * 32) == (9, 225, 16777216)
    assert got["draw"][0]["increments"] > 0


def draw_three_ways(cb, aref, oracle, cells, **kw):  # noqa: F811
    """The draw from a planted list: product == lock-step == restatement -> (restatement's counters, extra)."""
    s = aim.shape_of(kw)
    st = oracle.init_states(1337, 0, s["threads"])
    ex = {}
    want, wc = aim.draw(aref, cells, omp_threads=omp_threads(), states=st, extra=ex, **kw)
    for lockstep, kernel in BASES:
        hist, cnt, launched, after = gpu_draw(cb, lockstep, cells, **kw)
        assert launched == kernel
        same_counters(cnt, wc, (kernel, kw))
        assert np.array_equal(hist, want) and np.array_equal(after, planar_states(st)), (kernel, kw)
    return wc, ex


@pytest.mark.parametrize("case", [FIRST, BOUNDED, BOUNDED_JULIA, JULIA], ids=["plane", "bounded", "bounded_julia", "julia"])
def test_a_list_of_one_entry_and_the_whole_grid(cb, aref, oracle, case):  # noqa: F811
    mask, _ = aim.probe(aref, omp_threads=omp_threads(), **case)
    one = aim.cells(aref, mask, **dict(case, dilate=0))[:1]
    wc, ex = draw_three_ways(cb, aref, oracle, one, **case)
    assert wc["recorded"] > 0 and ex["in_canvas"] > 0  # every sample comes from a cell that reaches the canvas
    whole = np.arange(64 * 64, dtype=np.uint32)  # level 4: the sample plane itself, through the six-draw mapping
    wc, ex = draw_three_ways(cb, aref, oracle, whole, **dict(case, level=4))
    assert wc["recorded"] > 0


@pytest.mark.parametrize("threads", [1, 63, 64, 65, 255, 256, 257])
def test_thread_counts_around_a_wave_and_a_workgroup(cb, aref, oracle, threads):  # noqa: F811
    for case in (FIRST, BOUNDED_JULIA):
        mask, _ = aim.probe(aref, omp_threads=omp_threads(), **case)  # the common shape's list
        cells = aim.cells(aref, mask, **case)
        kw = dict(case, threads=threads, probe=(40,), draw=(60, 1))
        st = oracle.init_states(1337, 0, threads)
        want, pc = aim.probe(aref, states=st, **kw)
        for lockstep, kernel in BASES:
            got, cnt, launched, after = gpu_probe(cb, lockstep, **kw)
            assert launched == kernel and np.array_equal(got, want) and np.array_equal(after, planar_states(st))
            same_counters(cnt, pc, (kernel, threads))
        wc, _ = draw_three_ways(cb, aref, oracle, cells, **kw)
        assert wc["samples"] == 61 * threads


def test_launches_of_one_sample(cb, aref, oracle):  # noqa: F811
    for case in (FIRST, BOUNDED):
        got = three_ways(cb, aref, oracle, **dict(case, probe=(1,) * 16, draw=(1,) * 6))
        assert bits(got["mask"]) == aim.CASES["plane_zr_cr" if case is FIRST else "bounded_zr_cr"]["marked"]
        assert got["draw"][0]["samples"] == 6 * aim.THREADS


@pytest.mark.parametrize("max_iter", [0, 1, 59, 60, 61, 120, 121])
def test_a_bounded_max_at_the_chunk_boundaries(cb, aref, oracle, max_iter):  # noqa: F811
    for case in (BOUNDED, BOUNDED_JULIA):  # both sources of c
        got = three_ways(cb, aref, oracle, **dict(case, max_iter=max_iter))
        pc, pex = got["probe"]
        if max_iter == 0:  # nothing is tested and nothing plotted: every sample is bounded, none marks
            assert pc["never_escaped"] == pc["samples"] and pc["recorded"] == 0 and len(got["cells"]) == 0
            continue
        dc, dex = got["draw"]
        assert dc["recorded"] > 0 and dc["replay_steps"] == max_iter * dc["recorded"]
        assert (dex["cycles"] > 0) == (max_iter >= 120)  # a cycle needs a save and a later chunk boundary
