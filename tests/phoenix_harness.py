"""What the Phoenix render's GPU suites share (tests/test_gpu_phoenix.py, tests/test_gpu_planted_phoenix.py) -- test
infrastructure only: the launches through cb_draw_buddhabrot_phoenix, the CPU restatement of the same launches
(tests/phoenix_reference.c) and the three-way comparison product kernel (cb_debug_last_draw_kernel 24) == lock-step kernel
(25) == restatement.

Every function takes the shape as keywords over shape_of's defaults and, with `states`, an oracle state array
(tests/planted_samples.py plants its first samples) in the place of the fresh generators: on the device it is written over
them, the restatement advances a copy, and the array itself is left as it was."""

import numpy as np

import phoenix_reference as phoenix
import plot_harness
import plot_reference as plot
from plot_harness import DEPTH_SHAPE, SAME, SQUARE, omp_threads, planar_states

PRODUCT, LOCKSTEP = 24, 25
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE


def shape_of(kw):
    s = dict(w=W, h=H, box=SQUARE, max_iter=MAX, min_iter=MIN, threads=THREADS, launches=LAUNCHES, c=None,
             projection=plot.IDENTITY)
    s.update(kw)
    return s


def phoenix_launches(cb, variant, states=None, **kw):
    """`launches` on fresh generators, or on the given oracle `states` written over them, through
    cb_draw_buddhabrot_phoenix -> (hist [h, w], counters, kernel, states)."""
    s = shape_of(kw)
    bufs = plot_harness.Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"])
    if states is not None:
        plot_harness.write_states(bufs, states)
    return bufs.launches(cb.draw_buddhabrot_phoenix, s["launches"], variant,
                         iterations=cb.IterationControl(s["max_iter"], s["min_iter"]), projection=s["projection"],
                         julia_c=s["c"], phoenix_p=s["p"]).read()


def restated(pref, oracle, states=None, **kw):
    """The restatement of the same launches -> (hist, counters, discounts and cycles, generator states after)."""
    s = shape_of(kw)
    st = oracle.init_states(1337, 0, s["threads"]) if states is None else states.copy()
    assert len(st) == s["threads"]
    extra = {}
    hist, cnt = phoenix.draw(pref, s["w"], s["h"], s["max_iter"], s["min_iter"], s["threads"], list(s["launches"]),
                             p=s["p"], projection=s["projection"], c=s["c"], box=s["box"], omp_threads=omp_threads(),
                             states=st, extra=extra)
    assert cnt["samples"] == s["threads"] * sum(s["launches"]) and int(hist.sum()) == cnt["increments"]
    assert cnt["rejected"] == 0
    return hist, cnt, extra, planar_states(st)


def three_ways(cb, pref, oracle, states=None, **kw):
    """Product == lock-step == restatement -> (restatement's hist, counters, extra, the product's counters)."""
    planted = states
    want, wc, extra, states = restated(pref, oracle, planted, **kw)
    print("restatement", wc, extra)
    got = {}
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, after = phoenix_launches(cb, base, planted, **kw)
        print(kernel, cnt)
        assert launched == kernel
        assert cnt["status"] == 0
        assert {k: cnt[k] for k in SAME} == wc, (kernel, cnt, wc)
        assert hist.shape == want.shape and np.array_equal(hist, want), kernel
        assert np.array_equal(after, states), kernel
        assert cb.lib.cb_debug_interior_map_level() == 0  # no map, whatever p is
        got[kernel] = cnt
    assert got[LOCKSTEP]["skipped_steps"] == 0
    # no map and no table: the discount of the exact cycles found under the state rule is all skipped_steps contains
    assert got[PRODUCT]["skipped_steps"] == extra["skipped_state"], (got[PRODUCT], extra)
    return want, wc, extra, got[PRODUCT]
