"""What the period-palette render's GPU suites share (test_gpu_periods.py, test_gpu_periods_edges.py,
test_gpu_periods_fuzz.py) -- test infrastructure only: the fixture for the restatement (tests/period_reference.c), the
launches on the GPU through cb_draw_buddhabrot_periods on device_launches' buffers, and the three-way comparison product
kernel (28) == lock-step kernel (29) == restatement.  The shape and the cases' vocabulary are bounded_harness's.  A fixture
imported into a test module is a fixture of that module."""

import numpy as np
import pytest

import period_reference as period
import plot_reference as plot
from bounded_harness import KEYS, shape_of  # noqa: F401 (re-exported)
from plot_harness import SAME, Launches, omp_threads, planar_states, variant_of

PRODUCT, LOCKSTEP = 28, 29
NOT_INCREMENTS = [k for k in SAME if k != "increments"]


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return period.load(tmp_path_factory.mktemp("period_ref"))


def period_launches(cb, base, lut, eps=period.DEFAULT_EPS, **kw):
    """`launches` on fresh generators through cb_draw_buddhabrot_periods -> (hist [3, h, w], counters, kernel, states)."""
    s = shape_of(kw)
    bufs = Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"], planes=3, tables={"lut": lut})
    variant = variant_of(cb, base, s["degree"], s["ship"], plot.code_of(s["formula"]))
    return bufs.launches(cb.draw_buddhabrot_periods, s["launches"], variant,
                         iterations=cb.IterationControl(s["max_iter"], s["min_iter"]), projection=s["projection"],
                         julia_c=s["c"], d_lut=bufs.tables["lut"].data_ptr(), n_entries=bufs.tables["lut"].numel(),
                         period_eps=eps).read()


def restated(pref, oracle, lut, eps=period.DEFAULT_EPS, mode=period.NAIVE, **kw):
    """The restatement of the same launches -> (hist, counters, extra, generator states after)."""
    s = shape_of(kw)
    st = oracle.init_states(1337, 0, s["threads"])
    extra = {}
    hist, cnt = period.draw(pref, s["w"], s["h"], s["max_iter"], s["threads"], list(s["launches"]), lut, eps=eps,
                            projection=s["projection"], degree=s["degree"], ship=s["ship"], formula=s["formula"], c=s["c"],
                            box=s["box"], mode=mode, omp_threads=omp_threads(), states=st, extra=extra)
    assert cnt["samples"] == s["threads"] * sum(s["launches"]) and int(hist.sum()) == cnt["increments"]
    return hist, cnt, extra, planar_states(st)


def three_ways(cb, pref, oracle, lut, eps=period.DEFAULT_EPS, **kw):
    """Product == lock-step == restatement, bit for bit on the three planes, the generator states and the counters of SAME;
    the product's skipped_steps is the compressed restatement's, to the step -> (restatement's hist, counters, extra, the
    product's counters)."""
    want, wc, extra, states = restated(pref, oracle, lut, eps, **kw)
    compressed = restated(pref, oracle, lut, eps, mode=period.COMPRESSED, **kw)
    assert np.array_equal(compressed[0], want) and {k: compressed[1][k] for k in SAME} == {k: wc[k] for k in SAME}
    assert {k: compressed[2][k] for k in period.CLASSES} == {k: extra[k] for k in period.CLASSES}
    m = max(shape_of(kw)["max_iter"], 0)
    assert wc["rejected"] == 0 and wc["never_escaped"] == wc["recorded"] and wc["replay_steps"] == m * wc["recorded"]
    assert wc["recorded"] == sum(extra[k] for k in ("cycle_period", "cycle_none", "tol_period", "tol_none"))
    print("restatement", wc, extra, "compressed search steps", compressed[2]["search_steps"])
    got = {}
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, after = period_launches(cb, base, lut, eps, **kw)
        print(kernel, cnt)
        assert launched == kernel
        assert cnt["status"] == 0
        assert {k: cnt[k] for k in SAME} == {k: wc[k] for k in SAME}, (kernel, cnt, wc)
        assert hist.shape == want.shape and np.array_equal(hist, want), kernel
        assert np.array_equal(after, states), kernel
        assert int(hist.sum()) == cnt["increments"]
        assert cb.lib.cb_debug_interior_map_level() == 0  # no map, whatever the step
        got[kernel] = cnt
    assert got[LOCKSTEP]["skipped_steps"] == 0
    assert got[PRODUCT]["skipped_steps"] == compressed[1]["skipped_steps"], (got[PRODUCT], compressed[1])
    return want, wc, extra, got[PRODUCT]
