"""The palette render (include/cudabrot_amd.h, "Palette render") on the GPU.  Every case three ways -- the product kernel
(cb_debug_last_draw_kernel 14), the lock-step kernel (15), the CPU restatement (tests/plot_reference.c) -- bit for bit on
the three planes, the generator states and every counter but skipped_steps:

  1. the steps and both sources of c;
  2. the constant table against the renders without a palette;
  3. a table of windows against those renders window by window, and what a zero entry skips;
  4. the edges of the table;
  5. everything the ABI refuses;
  6. the renderer and its image;
  7. the binary.

The shape is small on purpose: w != h (a transposed plane stride shows), 1000 threads (a partial workgroup and a partial
wave), two launches on the same generators, and a table whose neighbours differ (an off-by-one in k shows)."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import INVALID, SAME, SQUARE, exe, omp_threads, planar_states, ref, variant_of  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 14, 15
W, H, MAX, MIN, THREADS, LAUNCHES = 250, 130, 500, 20, 1000, (3, 2)
C_JULIA = (-0.8, 0.156)
# parameters at which the other steps have orbits with k >= 20 among 5000 starting points (at C_JULIA they have none:
# every start escapes within a few steps there, and the case would compare empty planes)
C_CUBIC, C_SHIP = (0.4, 0.0), (0.3, 0.0)
WINDOWS = [(20, 60), (60, 200), (100, 500)]  # G and B overlap


def gpu_launches(cb, lut, variant, c=None, projection=plot.IDENTITY, w=W, h=H, box=SQUARE, max_iter=MAX, min_iter=MIN,
                 threads=THREADS, launches=LAUNCHES):
    """plot_harness.gpu_launches at this suite's shape.  lut None: the same render without a palette
    (cb_draw_buddhabrot_projected, or cb_draw_buddhabrot_julia with a c) -> hist [h, w]."""
    return plot_harness.gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, variant, c, lut, projection)


def three_ways(cb, ref, oracle, lut, c=None, degree=2, ship=False, projection=plot.IDENTITY, w=W, h=H, box=SQUARE,
               max_iter=MAX, min_iter=MIN, threads=THREADS, launches=LAUNCHES, device_lut=None):
    """Product == lock-step == restatement -> (restatement's hist, its counters, its zero-entry replay steps, the
    product's counters).  The product kernel consults the interior map where cb_draw_buddhabrot_projected does: the
    Mandelbrot step on a sampled c, max_iter above 20 (tests/test_gpu_project.py)."""
    map_level = 1 if c is None and degree == 2 and not ship and max_iter > 20 else 0
    r = plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), map_level, w, h, box, max_iter, min_iter, threads,
                                launches, degree=degree, ship=ship, c=c, lut=lut, device_lut=device_lut, projection=projection)
    return r.want, r.wc, r.extra["zero_entry_steps"], r.product


# ---- 1. the steps and both sources of c -------------------------------------------------------------------------------------

CASES = {
    "mandelbrot": dict(),
    "hologram_cropped": dict(projection=plot.HOLOGRAM, box=(-1.3, 0.9, -0.7, 0.55)),
    "ship": dict(ship=True),
    "degree3": dict(degree=3),
    "degree8": dict(degree=8),
    "julia": dict(c=C_JULIA),
    "julia_degree3": dict(c=C_CUBIC, degree=3),
    "julia_ship": dict(c=C_SHIP, ship=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_product_lockstep_and_restatement_agree(cb, ref, oracle, name):
    want, wc, _, _ = three_ways(cb, ref, oracle, plot.demo_table(MAX), **CASES[name])
    assert wc["recorded"] > 0 and wc["increments"] > wc["recorded"]  # weighted points
    assert want[0].any() and want[1].any() and want[2].any()
    assert (wc["rejected"] > 0) == (name in ("mandelbrot", "hologram_cropped"))  # cardioid and bulb: that step, sampled c


def test_the_mandelbrot_step_on_a_sampled_c_uses_the_interior_map(cb):
    lut = plot.demo_table(MAX)
    gpu_launches(cb, lut, cb.CB_KERNEL_DEFAULT)
    assert cb.lib.cb_debug_interior_map_level() > 0
    for kw in (dict(c=C_JULIA), dict(variant=cb.CB_KERNEL_SIMPLE), dict(variant=cb.CB_KERNEL_FLAG_BURNING_SHIP),
               dict(variant=cb.CB_KERNEL_POWER(3))):
        gpu_launches(cb, lut, kw.pop("variant", cb.CB_KERNEL_DEFAULT), **kw)
        assert cb.lib.cb_debug_interior_map_level() == 0


@pytest.mark.parametrize("degree", [4, 5, 6, 7])
@pytest.mark.parametrize("c", [None, (0.3, -0.2)], ids=["sampled", "fixed"])
def test_the_other_degrees_are_their_own_instances(cb, ref, oracle, degree, c):
    _, wc, _, _ = three_ways(cb, ref, oracle, plot.demo_table(100), c=c, degree=degree, max_iter=100, min_iter=0, w=64,
                             h=48, threads=300, launches=[4])
    assert wc["recorded"] > 0


# ---- 2. the constant table is the render without a palette ----------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_constant_table_equals_the_plain_render(cb, base, c):
    lut = np.full(MAX, 0x010101, dtype=np.uint32)
    hist, cnt, kernel, states = gpu_launches(cb, lut, base, c, plot.HOLOGRAM)
    plain, pc, plain_kernel, plain_states = gpu_launches(cb, None, base, c, plot.HOLOGRAM)
    assert kernel == (LOCKSTEP if base else PRODUCT) and plain_kernel == (8 if c is None else 12) + base
    assert pc["increments"] > 0
    for j in range(3):
        assert np.array_equal(hist[j], plain), j
    assert cnt["increments"] == 3 * pc["increments"]
    assert {k: cnt[k] for k in SAME if k != "increments"} == {k: pc[k] for k in SAME if k != "increments"}
    assert cnt["status"] == 0 and np.array_equal(states, plain_states)
    assert cnt["skipped_steps"] == pc["skipped_steps"]  # no entry is zero: nothing more is skipped


# ---- 3. windows -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("min_iter", [MIN, 5], ids=["every_k_in_a_window", "k_below_20_in_none"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_window_table_equals_the_plain_render_of_each_window(cb, ref, oracle, c, min_iter):
    lut = plot.window_table(MAX, WINDOWS)
    want, wc, zero_steps, product = three_ways(cb, ref, oracle, lut, c=c, min_iter=min_iter)
    hist, cnt, _, _ = gpu_launches(cb, lut, cb.CB_KERNEL_DEFAULT, c, min_iter=min_iter)
    for j, (lo, hi) in enumerate(WINDOWS):
        plain, pc, _, _ = gpu_launches(cb, None, cb.CB_KERNEL_DEFAULT, c, max_iter=hi, min_iter=lo)
        assert pc["increments"] > 0
        assert np.array_equal(hist[j], plain), j
    # what the zero entries skip: the same run under the constant table skips everything else the same way
    constant = np.full(MAX, 0x010101, dtype=np.uint32)
    _, cc, _, _ = gpu_launches(cb, constant, cb.CB_KERNEL_DEFAULT, c, min_iter=min_iter)
    assert (zero_steps > 0) == (min_iter < 20)
    assert product["skipped_steps"] - cc["skipped_steps"] == zero_steps
    assert cnt["skipped_steps"] == product["skipped_steps"]
    assert cc["recorded"] == wc["recorded"] and cc["replay_steps"] == wc["replay_steps"]  # zero entries still count


# ---- 4. edges of the table ---------------------------------------------------------------------------------------------------


def ends_only(n, lo):
    lut = np.zeros(n, dtype=np.uint32)
    lut[lo] = 0x000007
    lut[n - 1] = 0x050000
    return lut


EDGES = {
    "min0_reads_entry_0": dict(lut=plot.demo_table(MAX) | np.uint32(0x030000), min_iter=0),
    "max1": dict(lut=np.array([0x0a0b0c], dtype=np.uint32), max_iter=1, min_iter=0),
    "only_k_min_and_k_max_minus_1": dict(lut=ends_only(MAX, MIN)),
    "weights_255": dict(lut=np.full(MAX, 0xFFFFFF, dtype=np.uint32)),
    "julia_min0": dict(lut=plot.demo_table(60), c=C_JULIA, max_iter=60, min_iter=0),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(cb, ref, oracle, name):
    want, wc, zero_steps, product = three_ways(cb, ref, oracle, **EDGES[name])
    assert wc["recorded"] > 0 and wc["increments"] > 0
    if name == "max1":  # only k == 0: one replayed point each, weights 12, 11, 10
        assert wc["replay_steps"] == wc["recorded"] and want[0].sum() * 11 == want[1].sum() * 12
    elif name == "only_k_min_and_k_max_minus_1":
        assert want[0].any() and not want[1].any() and zero_steps > 0
        assert int(want[0].sum()) % 7 == 0 and int(want[2].sum()) % 5 == 0
    elif name == "weights_255":
        assert np.array_equal(want[0], want[1]) and np.array_equal(want[0], want[2]) and int(want[0].sum()) % 255 == 0


def test_bits_24_to_31_of_the_device_table_change_nothing(cb, ref, oracle):
    lut = plot.demo_table(MAX)
    lut[30:40] = 0  # zero entries stay zero entries under the high bits
    three_ways(cb, ref, oracle, lut, device_lut=lut | np.uint32(0xFF000000))
    three_ways(cb, ref, oracle, lut, c=C_JULIA, device_lut=lut | np.uint32(0x01000000))


# ---- 5. what the ABI refuses -------------------------------------------------------------------------------------------------


def test_palette_launches_refuse_what_they_do_not_define(cb):
    import torch

    dev = torch.device("cuda", 0)
    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    d_lut = torch.full((100,), 0x010101, dtype=torch.int32, device=dev)
    bufs = plot_harness.Launches(cb, dims, threads, planes=3)
    buf, counters, states = bufs.out, bufs.counters, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_matrix = (C.c_double * 8)(*([float("nan")] + list(cb.IDENTITY_PROJECTION[1:])))
    inf_matrix = (C.c_double * 8)(*(list(cb.IDENTITY_PROJECTION[:7]) + [float("inf")]))
    c_good = (C.c_double * 2)(*C_JULIA)
    d, b, s, k = C.byref(dims), buf.data_ptr(), states.data_ptr(), counters.data_ptr()

    def draw(variant=0, c=None, p=good, lut=d_lut.data_ptr(), n=100, iterations=it, samples=5, n_threads=threads):
        return cb.lib.cb_draw_buddhabrot_palette(d, b, C.byref(iterations), p, c, lut, n, s, n_threads, samples, k, variant,
                                                 None)

    for c in (None, c_good):
        assert draw(c=c, lut=None) == INVALID  # a NULL table
        for n in (99, 101, 0, (1 << 24) + 1):  # not max, none, more than the largest table
            assert draw(c=c, n=n) == INVALID, n
        for m, n in ((0, 0), ((1 << 24) + 1, (1 << 24) + 1), (-3, 100)):
            assert draw(c=c, n=n, iterations=cb.IterationControl(m, 0)) == INVALID, m
        assert draw(c=c, p=None) == INVALID and draw(c=c, p=bad_matrix) == INVALID and draw(c=c, p=inf_matrix) == INVALID
        power3 = cb.CB_KERNEL_POWER(3)
        bad_variants = [cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_TIMED,
                        cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_DRAIN, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        power3 | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP, power3 | cb.CB_KERNEL_FLAG_ANTI,
                        2 << 12, 9 << 12, 15 << 12]
        for variant in bad_variants:
            assert draw(variant, c=c) == INVALID, variant
    nan, inf = float("nan"), float("inf")
    for c in ((2.5, 0.0), (0.0, 2.5), (-2.0000001, 0.0), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=(C.c_double * 2)(*c)) == INVALID, c
    assert cb.lib.cb_draw_buddhabrot_palette(None, b, C.byref(it), good, None, d_lut.data_ptr(), 100, s, threads, 5, k, 0,
                                             None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_palette(d, None, C.byref(it), good, None, d_lut.data_ptr(), 100, s, threads, 5, k, 0,
                                             None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_palette(d, b, C.byref(it), good, None, d_lut.data_ptr(), 100, None, threads, 5, k, 0,
                                             None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        for c in (None, c_good):
            assert draw(base, c=c, samples=0) == 0 and draw(base, c=c, n_threads=0) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)


def test_renderer_refuses_a_palette_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(*C_JULIA)
    lut = np.full(100, 0x010203, dtype=np.uint32)

    def set_palette(r, table=lut, n=None):
        return cb.lib.cb_renderer_set_palette(r._h, None if table is None else table.ctypes.data,
                                              (0 if table is None else table.size) if n is None else n)

    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert set_palette(r) == INVALID and r.palette() is None  # a channel renderer
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert set_palette(r, np.full(300, 1, dtype=np.uint32)) == INVALID  # a focused renderer
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.render_passes(1)
        assert set_palette(r) == INVALID  # after the first pass
        assert r.read_histogram().shape == (64, 64)
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        fresh = r.read_rng_states().copy()
        n = C.c_uint32(77)
        assert cb.lib.cb_renderer_palette(r._h, C.byref(n)) == 0 and n.value == 77
        assert set_palette(r, None, 100) == INVALID
        assert set_palette(r, lut[:99]) == INVALID and set_palette(r, np.full(101, 1, dtype=np.uint32)) == INVALID
        assert set_palette(r, lut, 0) == INVALID
        high = lut.copy()
        high[99] |= 0x01000000
        assert set_palette(r, high) == INVALID  # a bit of 24 .. 31
        rgb = np.zeros((64, 64, 3), dtype=">u2")
        assert cb.lib.cb_renderer_palette_image(r._h, 1.0, 0, rgb.ctypes.data, None, None) == INVALID  # no palette yet
        assert r.palette() is None and r.projection() is None and r.read_histogram().shape == (64, 64)
        r.set_palette(lut)  # alone: the identity projection
        assert r.palette() == 100 and np.array_equal(r.projection().reshape(-1), np.array(cb.IDENTITY_PROJECTION))
        assert r.julia() is None
        assert set_palette(r) == INVALID  # once
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FULL_ITERATE, 9 << 12,
                        cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        hist = r.read_histogram()
        assert hist.shape == (3, 64, 64) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        assert cb.lib.cb_renderer_palette_image(r._h, 1.0, 0, None, None, None) == INVALID
        assert cb.lib.cb_renderer_palette_image(r._h, 1.0, 7, rgb.ctypes.data, None, None) == INVALID  # no such tone mode
    assert cb.lib.cb_renderer_set_palette(None, lut.ctypes.data, 100) == INVALID
    with cb.Renderer(dims, cb.IterationControl(0, 0), device=0, n_threads=1024) as r:
        assert set_palette(r, lut, 0) == INVALID  # -m 0 has no table


# ---- 6. the renderer and its image -------------------------------------------------------------------------------------------


def host_image(cb, hist, gamma):
    """The header's Image rule on the host: the three planes as one w x 3h image, then interleaved -> ([h, w, 3] big-endian
    u16, max, scale)."""
    planes, h, w = hist.shape
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(3 * h, w), gamma)
    return np.ascontiguousarray(gray.reshape(3, h, w).transpose(1, 2, 0)).astype(">u2"), mx, scale


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("kind", ["projected", "julia_degree3", "alone"])
def test_palette_renderer_over_several_calls(cb, ref, oracle, base, kind):
    box, m, mn = (-2.0, 1.0, -1.5, 1.5), 300, 10
    c = C_CUBIC if kind == "julia_degree3" else None
    degree = 3 if kind == "julia_degree3" else 2
    p = plot.IDENTITY if kind == "alone" else plot.HOLOGRAM
    variant = variant_of(cb, base, degree)
    lut = plot.demo_table(m)
    lut[50:70] = 0
    st = oracle.init_states(1337, 0, THREADS)
    want, wc = plot.draw(ref, W, H, m, mn, THREADS, [50] * 3, lut=lut, c=c, degree=degree, projection=p, box=box,
                         omp_threads=omp_threads(), states=st)
    dims = cb.FractalDimensions.make(W, H, *box)
    with cb.Renderer(dims, cb.IterationControl(m, mn), device=0, n_threads=THREADS) as r:
        if kind == "projected":
            r.set_projection(p)
        elif kind == "julia_degree3":
            r.set_julia(c, p)
        r.set_palette(lut)
        r.prepare(variant)  # must not fail
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(2, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        states = r.read_rng_states().view(np.uint32)
        assert r.julia() == c
    assert wc["recorded"] > 100 and wc["increments"] > 100  # not empty
    assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == wc, (cnt, wc)
    assert hist.shape == (3, H, W) and np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))


@pytest.fixture(scope="module")
def rendered(cb):
    """One palette renderer with a few passes in it, and its histogram."""
    dims = cb.FractalDimensions.make(W, H)
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        r.set_palette(plot.demo_table(MAX))
        r.render_passes(3)
        yield r, r.read_histogram()


@pytest.mark.parametrize("mode", ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"])
@pytest.mark.parametrize("gamma", [1.0, 2.2, -1.0])
def test_palette_image_equals_the_host_computation(cb, rendered, mode, gamma):
    r, hist = rendered
    assert len({int(hist[j].max()) for j in range(3)}) == 3  # three different maxima: a common one shows
    rgb, mx, scale = r.palette_image(gamma, getattr(cb, mode))
    want, want_max, want_scale = host_image(cb, hist, gamma)
    assert mx == want_max == int(hist.max()) and scale == want_scale
    assert rgb.shape == (H, W, 3) and rgb.tobytes() == want.tobytes()
    assert int(rgb.max()) == 65535


def test_planes_of_a_palette_renderer_tone_map_with_their_own_maximum(cb, rendered):
    r, hist = rendered
    for j in range(3):
        gray, mx, _ = r.grayscale_image(1.0, plane=j)
        want, want_max, _ = cb.set_grayscale_pixels(hist[j], 1.0)
        assert mx == want_max == int(hist[j].max()) and np.array_equal(gray.astype(np.uint16), want)
    out = np.zeros((H, W), dtype=">u2")
    assert cb.lib.cb_renderer_grayscale_plane(r._h, 3, 1.0, 0, out.ctypes.data, None, None) == INVALID


def test_write_then_read_round_trips_the_three_planes(cb):
    dims = cb.FractalDimensions.make(W, H)
    rng = np.random.default_rng(7)
    planes = rng.integers(0, 1 << 40, size=(3, H, W), dtype=np.uint64)
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        r.set_palette(plot.demo_table(MAX))
        r.write_histogram(planes)
        assert np.array_equal(r.read_histogram(), planes)
        with pytest.raises(ValueError):
            r.write_histogram(planes[0])
        r.render_passes(1)  # adds to what was written
        after = r.read_histogram()
        assert np.all(after >= planes) and int((after - planes).sum()) == r.read_counters().as_dict()["increments"] > 0


# ---- 7. the binary -----------------------------------------------------------------------------------------------------------


STOPS_TEXT = "20:000030,200:ff8000,499:ffffff"
STOPS = [(20, 0x00, 0x00, 0x30), (200, 0xFF, 0x80, 0x00), (499, 0xFF, 0xFF, 0xFF)]
SHAPE = ["-w", str(W), "-h", str(H), "-m", str(MAX), "-c", str(MIN)]


def test_cli_palette_buffer_image_and_resume(cb, exe, ref, tmp_path):
    lut = cb.palette_from_stops(STOPS, MAX)
    common = ["--palette", STOPS_TEXT, "-g", "2.2", *SHAPE]
    one_buf, one_side, one_ppm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.ppm")
    r = run(exe, "--passes", "2", "-s", one_buf, "--rng-state", one_side, "--stats", "-o", one_ppm, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saving image." in r.stdout and "Done! Output image saved: %s" % one_ppm in r.stdout
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"palette": [[20, "000030"], [200, "ff8000"], [499, "ffffff"]]}
    want, wc = plot.draw(ref, W, H, MAX, MIN, 512 * 512, [100], lut=lut, omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    assert wc["recorded"] > 100000
    assert np.array_equal(read_state_file(one_buf, H, W, planes=3), want)
    # the image: header and body of the host computation
    body, mx, scale = host_image(cb, want, 2.2)
    with open(one_ppm, "rb") as f:
        data = f.read()
    header = b"P6\n%d %d\n65535\n" % (W, H)
    assert data[:len(header)] == header and data[len(header):] == body.tobytes()
    assert "Max value: %d, scale: %f" % (mx, scale) in r.stdout
    # the reference's host loop gives the same file
    host_ppm = str(tmp_path / "host.ppm")
    assert run(exe, "--passes", "2", "--tonemap", "host", "-o", host_ppm, *common).returncode == 0
    with open(host_ppm, "rb") as f:
        assert f.read() == data
    # one pass, the two files written, then one more pass on them: the same run
    buf, side = str(tmp_path / "two.bin"), str(tmp_path / "two.rng")
    assert run(exe, "--passes", "1", "-s", buf, "--rng-state", side, "-o", os.devnull, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, "-o", str(tmp_path / "two.ppm"), *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 1 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (str(tmp_path / "two.ppm"), one_ppm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a


def test_cli_palette_with_julia_and_power_on_another_plane(cb, exe, ref, tmp_path):
    buf = str(tmp_path / "p.bin")
    r = run(exe, "--julia", "0.4,0", "--power", "3", "--plane", "zr,cr", "--palette", STOPS_TEXT, "--passes", "1",
            "--kernel", "simple", "-s", buf, "--stats", "-o", os.devnull, *SHAPE)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert json.loads(lines[1]) == {"power": 3} and "julia" in json.loads(lines[2]) and "palette" in json.loads(lines[3])
    want, wc = plot.draw(ref, W, H, MAX, MIN, 512 * 512, [50], lut=cb.palette_from_stops(STOPS, MAX), c=C_CUBIC, degree=3,
                         projection=plot.ZR_CR, omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc and stats["skipped_steps"] == 0
    assert wc["recorded"] > 10000
    assert np.array_equal(read_state_file(buf, H, W, planes=3), want)
