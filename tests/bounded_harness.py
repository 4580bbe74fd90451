"""What the bounded render's GPU suites share (test_gpu_bounded.py, test_gpu_bounded_edges.py, test_gpu_bounded_fuzz.py) --
test infrastructure only: the fixture for the restatement (tests/bounded_reference.c), the launches on the GPU through
cb_draw_buddhabrot_bounded on device_launches' buffers, and the three-way comparison product kernel (26) == lock-step
kernel (27) == restatement.  A fixture imported into a test module is a fixture of that module."""

import numpy as np
import pytest

import bounded_reference as bounded
import plot_reference as plot
from plot_harness import DEPTH_SHAPE, SAME, SQUARE, Launches, omp_threads, planar_states, variant_of, write_states

PRODUCT, LOCKSTEP = 26, 27
# 64 x 48, 1000 threads (a ragged last wave and workgroup), launches of 3, 50 and 1 samples on the same generators, -m 500
# (orbits cross several 60-step chunk boundaries); min_iter is not read
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE
KEYS = SAME + ("skipped_steps",)


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return bounded.load(tmp_path_factory.mktemp("bounded_ref"))


def shape_of(kw):
    """states: an oracle state array (tests/planted_samples.py plants its first samples) in the place of the fresh
    generators; it is left as it was."""
    s = dict(w=W, h=H, box=SQUARE, max_iter=MAX, min_iter=MIN, threads=THREADS, launches=LAUNCHES, c=None,
             projection=plot.IDENTITY, degree=2, ship=False, formula=0, states=None)
    s.update(kw)
    return s


def bounded_launches(cb, base, **kw):
    """`launches` on fresh generators (or the given states) through cb_draw_buddhabrot_bounded -> (hist [h, w], counters,
    kernel, states)."""
    s = shape_of(kw)
    bufs = Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"])
    if s["states"] is not None:
        write_states(bufs, s["states"])
    variant = variant_of(cb, base, s["degree"], s["ship"], plot.code_of(s["formula"]))
    return bufs.launches(cb.draw_buddhabrot_bounded, s["launches"], variant,
                         iterations=cb.IterationControl(s["max_iter"], s["min_iter"]), projection=s["projection"],
                         julia_c=s["c"]).read()


def restated(bref, oracle, mode=bounded.NAIVE, **kw):
    """The restatement of the same launches -> (hist, counters, extra, generator states after)."""
    s = shape_of(kw)
    st = oracle.init_states(1337, 0, s["threads"]) if s["states"] is None else s["states"].copy()
    extra = {}
    hist, cnt = bounded.draw(bref, s["w"], s["h"], s["max_iter"], s["threads"], list(s["launches"]),
                             projection=s["projection"], degree=s["degree"], ship=s["ship"], formula=s["formula"], c=s["c"],
                             box=s["box"], mode=mode, omp_threads=omp_threads(), states=st, extra=extra)
    assert cnt["samples"] == s["threads"] * sum(s["launches"]) and int(hist.sum()) == cnt["increments"]
    return hist, cnt, extra, planar_states(st)


def three_ways(cb, bref, oracle, **kw):
    """Product == lock-step == restatement, bit for bit on histogram, generator states and the counters of SAME; the
    product's skipped_steps is the compressed restatement's -> (restatement's hist, counters, extra, the product's
    counters)."""
    want, wc, extra, states = restated(bref, oracle, **kw)
    compressed = restated(bref, oracle, mode=bounded.COMPRESSED, **kw)
    assert np.array_equal(compressed[0], want) and {k: compressed[1][k] for k in SAME} == {k: wc[k] for k in SAME}
    m = max(shape_of(kw)["max_iter"], 0)
    assert wc["rejected"] == 0 and wc["never_escaped"] == wc["recorded"] and wc["replay_steps"] == m * wc["recorded"]
    print("restatement", wc, extra)
    got = {}
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, after = bounded_launches(cb, base, **kw)
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
