"""What the plotted renders' suites share (projected, Multibrot, Julia, palette, formula, depth, depth palette) -- test
infrastructure only: the fixtures for the restatement and the binary, the launches on the GPU, and the three-way
comparison product kernel == lock-step kernel == CPU restatement (tests/plot_reference.c).  A fixture imported into a test
module is a fixture of that module.

The launch scaffolding itself -- buffers, generators, the launches and the read-back -- is tools/gpu_launches.py's,
imported as device_launches and shared with every other GPU suite and with tools/gpu_fuzz.py; gpu_launches here only
picks the entry point and its arguments.  SAME, SQUARE, omp_threads, planar_states, run and gpu_run are re-exported from there for the plotted suites."""

import collections

import numpy as np
import pytest

import plot_reference as plot
from cli_harness import exe  # noqa: F401 (the binary's fixture, re-exported for the GPU suites)
from device_launches import SAME, SQUARE, Launches, gpu_run, omp_threads, planar_states, run  # noqa: F401 (re-exported)

assert SAME == plot.COUNTER_NAMES
INVALID = 1  # hipErrorInvalidValue
NOT_INCREMENTS = [k for k in SAME if k != "increments"]

# What the two depth suites share.  The shape, small on purpose: 64 x 48 (a transposed plane stride shows), 1000 threads (a
# ragged last wave and workgroup), launches of 3, 50 and 1 samples on the same generators, -m 500 -c 20 (orbits cross
# several 60-step chunk boundaries, so the exact-periodicity early-out is reached).
DEPTH_SHAPE = 64, 48, 500, 20, 1000, (3, 50, 1)  # w, h, max_iter, min_iter, threads, launches
C_JULIA = (-0.8, 0.156)
# the z_re axis turned by three angles: a unit row with four irrational entries
IRRATIONAL_ROW = plot.rotate(plot.rotate(plot.rotate(plot.IDENTITY, "zr", "zi", 25.0), "zr", "cr", 40.0), "zi", "ci", 55.0)[0]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return plot.load(tmp_path_factory.mktemp("plot_ref"))


def variant_of(cb, base, degree=2, ship=False, formula=0):
    return (base | (cb.CB_KERNEL_POWER(degree) if degree != 2 else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
            | (cb.CB_KERNEL_FORMULA(formula) if formula else 0))


def write_states(run, states):
    """An oracle state array (tests/planted_samples.py plants its first samples) written over the fresh generators of a
    Launches, as the library's six planes."""
    assert len(states) == run.threads
    run.states.copy_(run.torch.from_numpy(planar_states(states).view(np.uint8)).to(run.dev))


def gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, variant, c=None, lut=None, projection=plot.IDENTITY,
                 depth=None, depth_lut=None, states=None):
    """`launches` (samples per thread each) on fresh generators (seed 1337, subsequences [0, threads)), or on the given
    oracle `states` written over them (they are left as they were), through the entry
    point the arguments pick -- with depth = (row, min, max, slices) cb_draw_buddhabrot_depth_palette (depth_lut, a table
    of `slices` entries) or cb_draw_buddhabrot_depth; else cb_draw_buddhabrot_palette with a table, cb_draw_buddhabrot_julia
    with a c, else cb_draw_buddhabrot_projected, or, projection=None, the normal path: cb_draw_buddhabrot without workspace
    and carry -> (u64 hist [h, w], or [planes, h, w] with a table (3) or a depth (3 with its table, else slices), counters
    dict, cb_debug_last_draw_kernel, generator states as u32 planes)."""
    dd = None if depth is None else cb.Depth.make(*depth)
    assert lut is None if depth is not None else depth_lut is None  # a table by escape index under a depth is not defined
    lut = lut if depth is None else depth_lut
    planes = 3 if lut is not None else None if depth is None else dd.slices
    run = Launches(cb, cb.FractalDimensions.make(w, h, *box), threads, planes=planes,
                   tables={} if lut is None else {"lut": lut})
    if states is not None:
        write_states(run, states)
    args = dict(iterations=cb.IterationControl(max_iter, min_iter), projection=projection)
    if lut is not None:
        args.update(d_lut=run.tables["lut"].data_ptr(), n_entries=run.tables["lut"].numel())
    if depth is not None:
        entry = cb.draw_buddhabrot_depth if lut is None else cb.draw_buddhabrot_depth_palette
        args.update(julia_c=c, depth=dd)
    elif lut is not None or c is not None:
        entry = cb.draw_buddhabrot_julia if lut is None else cb.draw_buddhabrot_palette
        args.update(julia_c=c)
    elif projection is not None:
        entry = cb.draw_buddhabrot_projected
    else:
        entry = cb.draw_buddhabrot
        del args["projection"]
    return run.launches(entry, launches, variant, **args).read()


# want, wc: the restatement's histogram and counters; product, lockstep: the two kernels' counters; extra: the
# restatement's zero_entry_steps and chunk_repeats and, under a depth with a table, "planes": the N planes of the
# restatement of the same depth without the table
ThreeWays = collections.namedtuple("ThreeWays", "want wc product lockstep extra")


def three_ways(cb, ref, oracle, kernels, map_level, w, h, box, max_iter, min_iter, threads, launches, *, degree=2,
               ship=False, formula=0, c=None, lut=None, device_lut=None, projection=plot.IDENTITY, depth=None, states=None):
    """Product == lock-step == restatement, bit for bit on histogram, generator states and the counters of SAME.
    kernels: the family's (product, lock-step) values of cb_debug_last_draw_kernel.  map_level: 0, or the least
    interior-map level the product kernel's launch must report (the lock-step kernel's reports 0 always); None is
    cb_draw_buddhabrot_projected's rule, 1 exactly under the Mandelbrot step on a sampled c.  device_lut: the table the
    GPU is given where it is not `lut` itself.  depth: (row, min, max, slices); lut is then the table by slice.  states: an
    oracle state array (planted first samples) in the place of the fresh generators, left as it was; the rule that only the
    Mandelbrot step on a sampled c rejects then holds one way only (planted samples need not reach a shape)."""
    launches = list(launches)
    before = states
    st = oracle.init_states(1337, 0, threads) if before is None else before.copy()
    extra = {}
    kw = dict(projection=projection, degree=degree, ship=ship, formula=formula, c=c, box=box, omp_threads=omp_threads())
    want, wc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, lut=lut, depth=depth, states=st, extra=extra, **kw)
    assert wc["samples"] == threads * sum(launches) and int(want.sum()) == wc["increments"]
    assert want.shape == ((3, h, w) if lut is not None else (h, w) if depth is None else (depth[3], h, w))
    mandelbrot = c is None and not formula and degree == 2 and not ship
    # nothing is rejected but under the reference's own step on a sampled c
    assert (wc["rejected"] > 0) == mandelbrot or (before is not None and wc["rejected"] == 0)
    if map_level is None:
        map_level = 1 if mandelbrot else 0
    table = lut if device_lut is None else device_lut
    got = {}
    for base, kernel in zip((cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE), kernels):
        hist, cnt, launched, states = gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches,
                                                   variant_of(cb, base, degree, ship, formula), c,
                                                   table if depth is None else None, projection, depth,
                                                   None if depth is None else table, states=before)
        print(kernel, cnt)
        assert launched == kernel
        assert cnt["status"] == 0
        assert {k: cnt[k] for k in SAME} == wc, (kernel, cnt, wc)
        assert hist.shape == want.shape and np.array_equal(hist, want), kernel
        assert np.array_equal(states, planar_states(st)), kernel
        assert int(hist.sum()) == cnt["increments"]
        level = cb.lib.cb_debug_interior_map_level()
        if map_level and base == cb.CB_KERNEL_DEFAULT:
            assert level >= map_level, (kernel, level)
        else:
            assert level == 0, (kernel, level)
        got[kernel] = cnt
    product, lockstep = (got[k] for k in kernels)
    assert lockstep["skipped_steps"] == 0
    assert product["skipped_steps"] >= extra["zero_entry_steps"]
    if depth is not None:
        # the depth renders' executed-work discount: something is skipped exactly where the interior map or a sample the
        # restatement saw repeat a point at a chunk boundary offers it -- under a table too: nothing is skipped for a colour
        print("chunk_repeats", extra["chunk_repeats"], "product skipped_steps", product["skipped_steps"])
        assert extra["zero_entry_steps"] == 0
        if before is None:
            assert (product["skipped_steps"] > 0) == (mandelbrot or extra["chunk_repeats"] > 0)
    if depth is not None and lut is not None:  # against the restatement of the depth alone
        planes, vc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, depth=depth,
                               states=None if before is None else before.copy(), **kw)
        assert np.array_equal(want, plot.combine(lut, planes))
        assert {k: vc[k] for k in NOT_INCREMENTS} == {k: wc[k] for k in NOT_INCREMENTS}
        extra["planes"] = planes
    return ThreeWays(want, wc, product, lockstep, extra)
