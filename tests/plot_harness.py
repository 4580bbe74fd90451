"""What the plotted renders' suites share (projected, Multibrot, Julia, palette, formula) -- test infrastructure only: the
fixtures for the restatement and the binary, the launches on the GPU, and the three-way comparison product kernel ==
lock-step kernel == CPU restatement (tests/plot_reference.c).  A fixture imported into a test module is a fixture of that
module."""

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


def gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, variant, c=None, lut=None, projection=plot.IDENTITY):
    """`launches` (samples per thread each) on fresh generators (seed 1337, subsequences [0, threads)) through the entry
    point the arguments pick -- cb_draw_buddhabrot_palette with a table, cb_draw_buddhabrot_julia with a c, else
    cb_draw_buddhabrot_projected, or, projection=None, the normal path: cb_draw_buddhabrot without workspace and carry
    -> (u64 hist [h, w] or [3, h, w], counters dict, cb_debug_last_draw_kernel, generator states as u32 planes)."""
    import torch

    dev = torch.device("cuda", 0)
    dims = cb.FractalDimensions.make(w, h, *box)
    it = cb.IterationControl(max_iter, min_iter)
    counters = torch.zeros(17, dtype=torch.int64, device=dev)
    states = torch.empty(cb.rng_state_bytes(threads), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cb.initialize_rng(cb.CB_DEFAULT_RNG_SEED, 0, threads, states.data_ptr(), stream)
    planes = 1 if lut is None else 3
    out = torch.zeros(planes * w * h, dtype=torch.int64, device=dev)
    if lut is not None:
        table = np.ascontiguousarray(lut, dtype=np.uint32)
        d_lut = torch.from_numpy(table.view(np.int32).copy()).to(dev)
    for samples in launches:
        if lut is not None:
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
    return (hist.reshape(h, w) if lut is None else hist.reshape(3, h, w)), cnt, kernel, states.cpu().numpy().view(np.uint32)


# want, wc: the restatement's histogram and counters; product, lockstep: the two kernels' counters; extra: the
# restatement's zero_entry_steps and chunk_repeats
ThreeWays = collections.namedtuple("ThreeWays", "want wc product lockstep extra")


def three_ways(cb, ref, oracle, kernels, map_level, w, h, box, max_iter, min_iter, threads, launches, *, degree=2,
               ship=False, formula=0, c=None, lut=None, device_lut=None, projection=plot.IDENTITY):
    """Product == lock-step == restatement, bit for bit on histogram, generator states and the counters of SAME.
    kernels: the family's (product, lock-step) values of cb_debug_last_draw_kernel.  map_level: 0, or the least
    interior-map level the product kernel's launch must report (the lock-step kernel's reports 0 always).  device_lut:
    the table the GPU is given where it is not `lut` itself."""
    launches = list(launches)
    st = oracle.init_states(1337, 0, threads)
    extra = {}
    want, wc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, projection=projection, degree=degree, ship=ship,
                         formula=formula, c=c, lut=lut, box=box, omp_threads=omp_threads(), states=st, extra=extra)
    assert wc["samples"] == threads * sum(launches) and int(want.sum()) == wc["increments"]
    if c is not None or formula or degree != 2 or ship:  # nothing is rejected but under the reference's own step
        assert wc["rejected"] == 0
    got = {}
    for base, kernel in zip((cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE), kernels):
        hist, cnt, launched, states = gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches,
                                                   variant_of(cb, base, degree, ship, formula), c,
                                                   lut if device_lut is None else device_lut, projection)
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
    return ThreeWays(want, wc, product, lockstep, extra)
