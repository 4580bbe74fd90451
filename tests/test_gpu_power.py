"""The Multibrot render (include/cudabrot_amd.h, "Multibrot step") on the GPU.  Every case three ways -- the product
kernel (cb_debug_last_draw_kernel 10), the lock-step kernel (11), the CPU restatement (tests/plot_reference.c) -- bit for
bit on histogram, generator states and every counter but skipped_steps:

  1. every degree, whole and ragged grids, two launches on the same generators;
  2. the round and chunk edges of the scheduler (max_iter around 12 and 60) and of the accept filter;
  3. the exact-periodicity early-out fires and changes nothing but the executed work;
  4. other planes on a cropped canvas;
  5. everything the ABI refuses;
  6. the renderer and the binary.
"""

import ctypes as C
import json

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from plot_harness import SAME, SQUARE, exe, omp_threads, planar_states, ref  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 10, 11


def three_ways(cb, ref, oracle, w, h, box, max_iter, min_iter, threads, launches, degree, projection=plot.IDENTITY):
    """Product == lock-step == restatement, without an interior map -> plot_harness.ThreeWays."""
    return plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), 0, w, h, box, max_iter, min_iter, threads, launches,
                                   degree=degree, projection=projection)


# ---- 1. every degree ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("threads,launches", [(4096, [50]), (1000, [50, 7])], ids=["whole", "ragged"])
@pytest.mark.parametrize("degree", range(3, 9))
def test_every_degree(cb, ref, oracle, degree, threads, launches):
    wc = three_ways(cb, ref, oracle, 64, 64, SQUARE, 500, 20, threads, launches, degree).wc
    assert wc["samples"] == threads * sum(launches)
    assert wc["never_escaped"] > 0 and wc["too_fast"] > 0 and wc["recorded"] > 0 and wc["increments"] > wc["recorded"]


# ---- 2. round and chunk edges -------------------------------------------------------------------------------------------

# rounds are 12 steps and chunks 60 (draw_rounds.h): one below, at and one above each, and two chunks
EDGES = [(m, 0) for m in (0, 1, 11, 12, 13, 59, 60, 61, 120, 121)] + [(61, 60), (61, 61), (61, 66)]


@pytest.mark.parametrize("max_iter,min_iter", EDGES, ids=["m%d_c%d" % e for e in EDGES])
@pytest.mark.parametrize("degree", [3, 8])
def test_round_and_chunk_edges(cb, ref, oracle, degree, max_iter, min_iter):
    wc = three_ways(cb, ref, oracle, 64, 64, SQUARE, max_iter, min_iter, 1024, [20], degree).wc
    assert wc["samples"] == 1024 * 20
    if max_iter == 0:
        assert wc["never_escaped"] == wc["samples"] and wc["iterate_steps"] == 0
    if min_iter >= max_iter > 0:  # the accept filter min <= k < max is empty
        assert wc["recorded"] == 0 and wc["increments"] == 0 and wc["too_fast"] > 0
    elif min_iter == 0 and max_iter > 0:
        assert wc["recorded"] > 0 and wc["too_fast"] == 0
    if (max_iter, min_iter) == (61, 60):  # only k == 60 is accepted (of so few samples, possibly none)
        assert wc["replay_steps"] == 61 * wc["recorded"]


# ---- 3. the early-out fires ----------------------------------------------------------------------------------------------


def test_early_out_changes_only_the_executed_work(cb, ref, oracle):
    """max_iter 2000 at degree 3: checked with the restatement before this shape was chosen, 21 871 of the 204 800
    samples are bit for bit at an earlier chunk boundary's point at a multiple of 60 steps below max (at least 100 are
    asserted again below); no larger max_iter was needed."""
    _, wc, product, lockstep, extra = three_ways(cb, ref, oracle, 64, 64, SQUARE, 2000, 20, 4096, [50], 3)
    assert extra["chunk_repeats"] >= 100
    assert product["skipped_steps"] > 0

    def executed(c):
        return c["iterate_steps"] - c["skipped_steps"]

    assert executed(product) < executed(lockstep) == wc["iterate_steps"]


# ---- 4. other planes -------------------------------------------------------------------------------------------------------

MATRICES = {"zr_cr": plot.ZR_CR, "hologram": plot.HOLOGRAM}


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("degree", [3, 5])
def test_other_planes_on_a_cropped_canvas(cb, ref, oracle, degree, name):
    wc = three_ways(cb, ref, oracle, 333, 77, (-1.3, 0.9, -0.7, 0.55), 500, 20, 2048, [50], degree, MATRICES[name]).wc
    assert 0 < wc["increments"] < wc["replay_steps"]  # points on the canvas and points off it


# ---- 5. what the ABI refuses -------------------------------------------------------------------------------------------------


def test_a_degree_is_refused_wherever_it_is_not_defined(cb):
    import torch

    dev = torch.device("cuda", 0)
    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    windows = (cb.IterationControl * 2)(cb.IterationControl(100, 20), cb.IterationControl(50, 5))
    mask = torch.zeros(cb.focus_mask_bytes(6), dtype=torch.uint8, device=dev)
    cells = torch.zeros(4, dtype=torch.int32, device=dev)
    bufs = plot_harness.Launches(cb, dims, threads, planes=2, no_counters=True)
    buf, states = bufs.out, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    invalid = 1  # hipErrorInvalidValue
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    d, b, i, s = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr()
    power3 = cb.CB_KERNEL_POWER(3)
    # the projected draw: field values outside 3 .. 8, the other steps, the other base variants
    bad_variants = [v << 12 for v in (1, 2, 9, 10, 11, 12, 13, 14, 15)]
    bad_variants += [v | cb.CB_KERNEL_SIMPLE for v in bad_variants]
    for degree in range(3, 9):
        p = cb.CB_KERNEL_POWER(degree)
        bad_variants += [p | cb.CB_KERNEL_FLAG_BURNING_SHIP, p | cb.CB_KERNEL_FLAG_ANTI, p | cb.CB_KERNEL_TIMED,
                         p | cb.CB_KERNEL_FULL_ITERATE, p | cb.CB_KERNEL_FLAG_DRAIN,
                         p | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                         p | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI]
    for variant in bad_variants:
        assert cb.lib.cb_draw_buddhabrot_projected(d, b, i, good, s, threads, 5, None, variant, None) == invalid, variant
    # every other entry point
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        v = power3 | base
        assert cb.lib.cb_draw_buddhabrot(d, b, i, s, threads, 5, None, v, None, 0, None, None) == invalid
        assert cb.lib.cb_draw_buddhabrot_channels(d, b, windows, 2, s, threads, 5, None, v, None, 0, None, None) == invalid
        assert cb.lib.cb_focus_probe(d, i, s, threads, 5, 6, mask.data_ptr(), None, v, None) == invalid
        assert cb.lib.cb_draw_buddhabrot_focus(d, b, i, s, threads, 5, None, v, 0, None, 0, None) == invalid
        assert cb.lib.cb_draw_buddhabrot_focus(d, b, i, s, threads, 5, None, v, 6, cells.data_ptr(), 4, None) == invalid
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(mask.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # the renderer: no focus probe with a degree, no degree without a projection
    with cb.Renderer(dims, it, device=0, n_threads=threads) as r:
        fresh = r.read_rng_states().copy()
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, power3 | base) == invalid
            assert cb.lib.cb_renderer_render_passes(r._h, 1, power3 | base) == invalid
        assert r.focus_cells() == (0, 0)
        assert int(r.read_histogram().sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        r.set_projection(cb.IDENTITY_PROJECTION)  # still possible: nothing was rendered
        for variant in (2 << 12, 9 << 12, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP, power3 | cb.CB_KERNEL_FLAG_ANTI):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == invalid
        assert int(r.read_histogram().sum()) == 0
        assert np.array_equal(r.read_rng_states(), fresh)


# ---- 6. the renderer and the binary -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
def test_renderer_passes_equal_the_restatement(cb, ref, oracle, base):
    w, h, m, c, threads = 64, 64, 500, 20, 4096
    st = oracle.init_states(1337, 0, threads)
    want, wc = plot.draw(ref, w, h, m, c, threads, [50] * 3, degree=3, omp_threads=omp_threads(), states=st)
    dims = cb.FractalDimensions.make(w, h)
    variant = base | cb.CB_KERNEL_POWER(3)
    with cb.Renderer(dims, cb.IterationControl(m, c), device=0, n_threads=threads) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.prepare(variant)  # must not fail
        r.render_passes(3, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        states = r.read_rng_states().view(np.uint32)
    assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == wc, (cnt, wc)
    assert np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))


@pytest.mark.parametrize("plane", [None, "zr,cr"], ids=["identity", "zr_cr"])
def test_cli_power_image_equals_the_restatement(exe, ref, cb, oracle, tmp_path, plane):
    out = str(tmp_path / "x.pgm")
    extra = ["--plane", plane] if plane else []
    r = run(exe, "--power", "3", "-w", "64", "-h", "64", "-m", "100", "-c", "20", "--passes", "1", "-o", out, "--stats",
            *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    p = plot.ZR_CR if plane else plot.IDENTITY
    want, wc = plot.draw(ref, 64, 64, 100, 20, 512 * 512, [50], projection=p, degree=3, omp_threads=omp_threads())
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [float(x) for x in plot.matrix(p)]
    assert json.loads(lines[1]) == {"power": 3}
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    assert wc["increments"] > 100000
    gray, _, _ = cb.set_grayscale_pixels(want, 1.0)
    with open(out, "rb") as f:
        assert f.read() == oracle.encode_pgm(gray)  # the header, then the values byte-swapped
