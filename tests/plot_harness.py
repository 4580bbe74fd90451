"""What the plotted renders' suites share (projected, Multibrot, Julia, palette, formula, depth, depth palette) -- test
infrastructure only: the fixtures for the restatement and the binary, the launches on the GPU, and the three-way
comparison product kernel == lock-step kernel == CPU restatement (tests/plot_reference.c).  A fixture imported into a test
module is a fixture of that module."""

import collections
import os
import subprocess

import numpy as np
import pytest

import plot_reference as plot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = plot.COUNTER_NAMES  # every counter but skipped_steps, the clocks and status
SQUARE = (-2.0, 2.0, -2.0, 2.0)
INVALID = 1  # hipErrorInvalidValue
NOT_INCREMENTS = [k for k in SAME if k != "increments"]

# What the two depth suites share.  The shape, small on purpose: 64 x 48 (a transposed plane stride shows), 1000 threads (a
# ragged last wave and workgroup), launches of 3, 50 and 1 samples on the same generators, -m 500 -c 20 (orbits cross
# several 60-step chunk boundaries, so the exact-periodicity early-out is reached).
DEPTH_SHAPE = 64, 48, 500, 20, 1000, (3, 50, 1)  # w, h, max_iter, min_iter, threads, launches
C_JULIA = (-0.8, 0.156)
# the z_re axis turned by three angles: a unit row with four irrational entries
IRRATIONAL_ROW = plot.rotate(plot.rotate(plot.rotate(plot.IDENTITY, "zr", "zi", 25.0), "zr", "cr", 40.0), "zi", "ci", 55.0)[0]


def omp_threads():
    v = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    return int(v) if v.isdigit() and int(v) > 0 else 16


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return plot.load(tmp_path_factory.mktemp("plot_ref"))


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "cudabrot")
    if not os.access(path, os.X_OK):
        pytest.fail("./cudabrot is not built (run `make` or __graft_entry__.build())")
    return path


def run(exe, *args, timeout=120, **kw):
    """The binary where it touches no device, or ends at once on a box without one."""
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, **kw)


def gpu_run(exe, *args):
    """The binary where it renders."""
    return run(exe, *args, timeout=600)


def planar_states(states):
    """The oracle's generator states (d, x[5]) as the library's six planes x0 .. x4, d."""
    return np.concatenate([states["x"][:, j] for j in range(5)] + [states["d"]]).astype(np.uint32)


def variant_of(cb, base, degree=2, ship=False, formula=0):
    return (base | (cb.CB_KERNEL_POWER(degree) if degree != 2 else 0) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
            | (cb.CB_KERNEL_FORMULA(formula) if formula else 0))


def gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, variant, c=None, lut=None, projection=plot.IDENTITY,
                 depth=None, depth_lut=None):
    """`launches` (samples per thread each) on fresh generators (seed 1337, subsequences [0, threads)) through the entry
    point the arguments pick -- with depth = (row, min, max, slices) cb_draw_buddhabrot_depth_palette (depth_lut, a table
    of `slices` entries) or cb_draw_buddhabrot_depth; else cb_draw_buddhabrot_palette with a table, cb_draw_buddhabrot_julia
    with a c, else cb_draw_buddhabrot_projected, or, projection=None, the normal path: cb_draw_buddhabrot without workspace
    and carry -> (u64 hist [h, w], or [planes, h, w] with a table (3) or a depth (3 with its table, else slices), counters
    dict, cb_debug_last_draw_kernel, generator states as u32 planes)."""
    import torch

    dev = torch.device("cuda", 0)
    dims = cb.FractalDimensions.make(w, h, *box)
    it = cb.IterationControl(max_iter, min_iter)
    counters = torch.zeros(17, dtype=torch.int64, device=dev)
    states = torch.empty(cb.rng_state_bytes(threads), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cb.initialize_rng(cb.CB_DEFAULT_RNG_SEED, 0, threads, states.data_ptr(), stream)
    dd = None if depth is None else cb.Depth.make(*depth)
    assert lut is None if depth is not None else depth_lut is None  # a table by escape index under a depth is not defined
    lut = lut if depth is None else depth_lut
    planes = 3 if lut is not None else 1 if depth is None else dd.slices
    out = torch.zeros(planes * w * h, dtype=torch.int64, device=dev)
    if lut is not None:
        table = np.ascontiguousarray(lut, dtype=np.uint32)
        d_lut = torch.from_numpy(table.view(np.int32).copy()).to(dev)
    for samples in launches:
        if depth is not None and lut is not None:
            cb.draw_buddhabrot_depth_palette(dims, out.data_ptr(), it, projection, c, dd, d_lut.data_ptr(), table.size,
                                             states.data_ptr(), threads, samples, counters.data_ptr(), variant, stream)
        elif depth is not None:
            cb.draw_buddhabrot_depth(dims, out.data_ptr(), it, projection, c, dd, states.data_ptr(), threads, samples,
                                     counters.data_ptr(), variant, stream)
        elif lut is not None:
            cb.draw_buddhabrot_palette(dims, out.data_ptr(), it, projection, c, d_lut.data_ptr(), table.size,
                                       states.data_ptr(), threads, samples, counters.data_ptr(), variant, stream)
        elif c is not None:
            cb.draw_buddhabrot_julia(dims, out.data_ptr(), it, projection, c, states.data_ptr(), threads, samples,
                                     counters.data_ptr(), variant, stream)
        elif projection is not None:
            cb.draw_buddhabrot_projected(dims, out.data_ptr(), it, projection, states.data_ptr(), threads, samples,
                                         counters.data_ptr(), variant, stream)
        else:
            cb.draw_buddhabrot(dims, out.data_ptr(), it, states.data_ptr(), threads, samples, counters.data_ptr(), variant,
                               stream)
    kernel = cb.lib.cb_debug_last_draw_kernel()
    torch.cuda.synchronize()
    names = [f[0] for f in cb.Counters._fields_]
    v = counters.cpu().numpy().view(np.uint64)
    cnt = {n: int(v[k]) for k, n in enumerate(names)}
    hist = out.cpu().numpy().view(np.uint64)
    hist = hist.reshape(h, w) if planes == 1 and depth is None else hist.reshape(planes, h, w)
    return hist, cnt, kernel, states.cpu().numpy().view(np.uint32)


# want, wc: the restatement's histogram and counters; product, lockstep: the two kernels' counters; extra: the
# restatement's zero_entry_steps and chunk_repeats and, under a depth with a table, "planes": the N planes of the
# restatement of the same depth without the table
ThreeWays = collections.namedtuple("ThreeWays", "want wc product lockstep extra")


def three_ways(cb, ref, oracle, kernels, map_level, w, h, box, max_iter, min_iter, threads, launches, *, degree=2,
               ship=False, formula=0, c=None, lut=None, device_lut=None, projection=plot.IDENTITY, depth=None):
    """Product == lock-step == restatement, bit for bit on histogram, generator states and the counters of SAME.
    kernels: the family's (product, lock-step) values of cb_debug_last_draw_kernel.  map_level: 0, or the least
    interior-map level the product kernel's launch must report (the lock-step kernel's reports 0 always); None is
    cb_draw_buddhabrot_projected's rule, 1 exactly under the Mandelbrot step on a sampled c.  device_lut: the table the
    GPU is given where it is not `lut` itself.  depth: (row, min, max, slices); lut is then the table by slice."""
    launches = list(launches)
    st = oracle.init_states(1337, 0, threads)
    extra = {}
    kw = dict(projection=projection, degree=degree, ship=ship, formula=formula, c=c, box=box, omp_threads=omp_threads())
    want, wc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, lut=lut, depth=depth, states=st, extra=extra, **kw)
    assert wc["samples"] == threads * sum(launches) and int(want.sum()) == wc["increments"]
    assert want.shape == ((3, h, w) if lut is not None else (h, w) if depth is None else (depth[3], h, w))
    mandelbrot = c is None and not formula and degree == 2 and not ship
    assert (wc["rejected"] > 0) == mandelbrot  # nothing is rejected but under the reference's own step on a sampled c
    if map_level is None:
        map_level = 1 if mandelbrot else 0
    table = lut if device_lut is None else device_lut
    got = {}
    for base, kernel in zip((cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE), kernels):
        hist, cnt, launched, states = gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches,
                                                   variant_of(cb, base, degree, ship, formula), c,
                                                   table if depth is None else None, projection, depth,
                                                   None if depth is None else table)
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
        assert (product["skipped_steps"] > 0) == (mandelbrot or extra["chunk_repeats"] > 0)
    if depth is not None and lut is not None:  # against the restatement of the depth alone
        planes, vc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, depth=depth, **kw)
        assert np.array_equal(want, plot.combine(lut, planes))
        assert {k: vc[k] for k in NOT_INCREMENTS} == {k: wc[k] for k in NOT_INCREMENTS}
        extra["planes"] = planes
    return ThreeWays(want, wc, product, lockstep, extra)
