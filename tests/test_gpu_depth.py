"""The depth render (include/cudabrot_amd.h, "Depth render") on the GPU:

  1. every case three ways -- the product kernel (cb_debug_last_draw_kernel 18), the lock-step kernel (19), the CPU
     restatement (tests/plot_reference.c) -- bit for bit on the N planes, the generator states and every counter but
     skipped_steps;
  2. against the projected and Julia renders, which are proven against the CPU on their own: no restatement involved;
  3. the renderer, its refusals and its image;
  4. the binary.

The shape is small on purpose: 64 x 48 (a transposed plane stride shows), 1000 threads (a ragged last wave and
workgroup), launches of 3, 50 and 1 samples on the same generators, -m 500 -c 20 (orbits cross several 60-step chunk
boundaries, so the exact-periodicity early-out is reached).

skipped_steps of the product kernel: above zero wherever there is something to skip -- the interior map (the Mandelbrot
step on a sampled c) or a sample the restatement saw repeat a point bit for bit at a chunk boundary.  The Julia set of
c = (-0.8, 0.156) has no such sample at this shape (its 211 never-escaping samples of 54000 are slow escapers, measured on
the CPU), so there the assertion is that nothing is skipped."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import C_JULIA, DEPTH_SHAPE, INVALID, IRRATIONAL_ROW, SAME, SQUARE  # noqa: F401
from plot_harness import exe, omp_threads, planar_states, ref, variant_of  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 18, 19
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE


def gpu_launches(cb, variant, c=None, projection=plot.IDENTITY, depth=None, w=W, h=H, box=SQUARE):
    """plot_harness.gpu_launches at this suite's shape: through cb_draw_buddhabrot_depth -> hist [slices, h, w], or,
    depth None, the same launches through cb_draw_buddhabrot_projected, or cb_draw_buddhabrot_julia with a c -> [h, w]."""
    return plot_harness.gpu_launches(cb, w, h, box, MAX, MIN, THREADS, LAUNCHES, variant, c, None, projection, depth)


def three_ways(cb, ref, oracle, d, *, box=SQUARE, **kw):
    """plot_harness.three_ways at this suite's shape -> (the restatement's histogram, its counters, the product's
    counters)."""
    r = plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), None, W, H, box, MAX, MIN, THREADS, LAUNCHES, depth=d,
                                **kw)
    return r.want, r.wc, r.product


# ---- 1. three ways ------------------------------------------------------------------------------------------------------

CASES = {
    # a non-dyadic delta_d (the division).  Hardly an accepted orbit has a c_re outside [-1.5, 0.5), so the points outside
    # the window at both ends are the second case's, whose window is cut inside the first's; likewise for the dyadic pair
    "mandelbrot_cr_5": dict(d=("cr", -2.0, 0.5, 5)),
    "mandelbrot_cr_inner": dict(d=("cr", -0.9, 0.0, 5)),
    "mandelbrot_zi_4_dyadic": dict(d=("zi", -2.0, 2.0, 4)),  # the reciprocal
    "mandelbrot_zi_inner_dyadic": dict(d=("zi", -0.5, 0.5, 8)),
    "hologram_irrational_row": dict(d=(IRRATIONAL_ROW, -0.9, 1.3, 7), projection=plot.HOLOGRAM),
    "ship": dict(d=("zi", -1.5, 1.2, 3), ship=True),
    "power_3": dict(d=("cr", -1.0, 1.0, 7), degree=3),
    "tricorn": dict(d=("zr", -2.0, 0.5, 5), formula=1),
    "julia_z_axis": dict(d=("zi", -1.0, 1.1, 6), c=C_JULIA),
}


@pytest.mark.parametrize("name", list(CASES))
def test_product_lockstep_and_restatement_agree(cb, ref, oracle, name):
    kw = dict(CASES[name])
    d = kw.pop("d")
    want, wc, product = three_ways(cb, ref, oracle, d, **kw)
    assert wc["recorded"] > 0 and 0 < wc["increments"] < wc["replay_steps"]  # some points are dropped
    assert sum(bool(p.any()) for p in want) >= 2  # and the rest spread over slices
    if name in ("mandelbrot_cr_inner", "mandelbrot_zi_inner_dyadic"):
        # points beyond both ends of the window: the wider window of the case before holds more at either end
        wider = CASES["mandelbrot_cr_5" if name == "mandelbrot_cr_inner" else "mandelbrot_zi_4_dyadic"]["d"]
        outer, oc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, depth=wider, omp_threads=omp_threads())
        lo, hi = d[1], d[2]
        edges = wider[1] + np.arange(wider[3] + 1) * ((wider[2] - wider[1]) / wider[3])
        below = sum(int(outer[s].sum()) for s in range(wider[3]) if edges[s + 1] <= lo)
        above = sum(int(outer[s].sum()) for s in range(wider[3]) if edges[s] >= hi)
        assert below > 0 and above > 0 and oc["increments"] - wc["increments"] >= below + above


def test_julia_on_a_c_axis_has_one_depth(cb, ref, oracle):
    """The depth of every point is that of the fixed c: all of them in one slice, or none in any."""
    want, wc, _ = three_ways(cb, ref, oracle, ("cr", -2.0, 0.5, 5), c=C_JULIA)
    s = int((C_JULIA[0] + 2.0) / 0.5)
    assert wc["increments"] > 0 and int(want[s].sum()) == wc["increments"]
    want, wc, _ = three_ways(cb, ref, oracle, ("ci", 0.2, 1.0, 3), c=C_JULIA)  # c_im = 0.156 is below the window
    assert wc["increments"] == 0 and wc["recorded"] > 0 and wc["replay_steps"] > 0
    # a row over both: K_d from the fixed c moves the window of z_im
    three_ways(cb, ref, oracle, ((0.0, 1.0, 0.5, -2.0), -1.0, 1.0, 4), c=C_JULIA)


# ---- 2. against the projected and Julia renders ---------------------------------------------------------------------------

# |z_0|^2 <= 8 and every later point follows one with |z|^2 <= 4: every visited coordinate of a degree-2 step is below
# 8 + 2 sqrt 2 < 16 in magnitude, of degree 3 below (2 sqrt 2)^3 + 2 sqrt 2 < 32.  64 slices: delta_d = 1/2 and 1.
COVERING = {
    "mandelbrot": dict(d=("zr", -16.0, 16.0, 64)),
    "mandelbrot_c_axis": dict(d=("ci", -16.0, 16.0, 64), projection=plot.HOLOGRAM),
    "power_3": dict(d=("zi", -32.0, 32.0, 64), degree=3),
    "julia": dict(d=("zi", -16.0, 16.0, 64), c=C_JULIA),
}


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", list(COVERING))
def test_slices_of_a_covering_window_sum_to_the_plain_render(cb, name, base):
    kw = dict(COVERING[name])
    d = kw.pop("d")
    variant = variant_of(cb, base, kw.pop("degree", 2))
    hist, cnt, kernel, states = gpu_launches(cb, variant, depth=d, **kw)
    plain, pc, plain_kernel, plain_states = gpu_launches(cb, variant, **kw)
    assert kernel == PRODUCT + base and plain_kernel in (8 + base, 10 + base, 12 + base)
    assert pc["increments"] > 0 and cnt["status"] == 0
    assert np.array_equal(hist.sum(axis=0), plain)  # also the check that the window covers
    assert {k: cnt[k] for k in SAME} == {k: pc[k] for k in SAME}
    assert cnt["skipped_steps"] == pc["skipped_steps"]  # the same early-outs, the same map
    assert np.array_equal(states, plain_states)
    assert sum(bool(p.any()) for p in hist) >= 2


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_one_slice_of_a_covering_window_is_the_plain_render(cb, c, base):
    hist, cnt, _, _ = gpu_launches(cb, base, c, plot.HOLOGRAM, ("cr", -16.0, 16.0, 1))
    plain, pc, _, _ = gpu_launches(cb, base, c, plot.HOLOGRAM)
    assert hist.shape == (1, H, W) and pc["increments"] > 0 and np.array_equal(hist[0], plain)
    assert {k: cnt[k] for k in SAME} == {k: pc[k] for k in SAME}


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("window", [(-2.0, 0.5, 5), (-1.0, 1.0, 8), (-1.3, 0.7, 48)], ids=["division", "reciprocal", "48"])
def test_the_slice_arithmetic_is_the_row_arithmetic(cb, window, base):
    """On a canvas of one row whose v window holds everything, the N slices of the depth render with rows (u; depth d) are
    the N rows of the projected render of the matrix (u-row, d-row) whose v window is the depth window: the slice is
    pixel_of's row, by either path."""
    lo, hi, n = window
    u_row, d_row = plot.HOLOGRAM[0], IRRATIONAL_ROW
    v_row = np.array([0.0, 1.0, 0.0, 0.0])
    hist, cnt, _, _ = gpu_launches(cb, base, None, np.vstack([u_row, v_row]), (d_row, lo, hi, n), h=1,
                                   box=(-2.0, 2.0, -16.0, 16.0))
    rows, rc, _, _ = gpu_launches(cb, base, None, np.vstack([u_row, d_row]), h=n, box=(-2.0, 2.0, lo, hi))
    assert hist.shape == (n, 1, W) and rows.shape == (n, W)
    assert 0 < rc["increments"] < rc["replay_steps"] and np.array_equal(hist[:, 0, :], rows)
    assert {k: cnt[k] for k in SAME} == {k: rc[k] for k in SAME}


# ---- 3. the renderer ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("kind", ["projected", "julia_power_3"])
def test_renderer_resumed_from_its_files_equals_one_run(cb, ref, oracle, base, kind):
    c, degree = ((0.4, 0.0), 3) if kind == "julia_power_3" else (None, 2)
    d = ("zi", -1.0, 1.1, 6)
    variant = variant_of(cb, base, degree)
    dims = cb.FractalDimensions.make(W, H)
    it = cb.IterationControl(300, 10)

    def renderer():
        r = cb.Renderer(dims, it, device=0, n_threads=THREADS)
        if c is None:
            r.set_projection(plot.HOLOGRAM)
        else:
            r.set_julia(c, plot.HOLOGRAM)
        assert r.depth() is None
        r.set_depth(d)
        return r

    with renderer() as one:
        one.prepare(variant)  # must not fail
        one.render_passes(3, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT + base
        want, wc, want_states = one.read_histogram(), one.read_counters().as_dict(), one.read_rng_states().copy()
        assert one.depth().as_tuple() == ((0.0, 1.0, 0.0, 0.0), -1.0, 1.1, 6)
        raw = cb.Depth()
        assert cb.lib.cb_renderer_depth(one._h, C.byref(raw)) == 6 and raw.as_tuple() == one.depth().as_tuple()
        assert cb.lib.cb_renderer_depth(one._h, None) == 6
    with renderer() as first:
        first.render_passes(2, variant)
        hist, states = first.read_histogram(), first.read_rng_states().copy()
    assert hist.shape == (6, H, W)
    with renderer() as second:
        second.write_histogram(hist)
        second.write_rng_states(states)
        with pytest.raises(ValueError):
            second.write_histogram(hist[0])
        second.render_passes(1, variant)
        got, got_states = second.read_histogram(), second.read_rng_states()
    assert wc["status"] == 0 and wc["increments"] > 100 and int(want.sum()) == wc["increments"]
    assert np.array_equal(got, want) and np.array_equal(got_states, want_states)
    st = oracle.init_states(1337, 0, THREADS)
    ref_hist, rc = plot.draw(ref, W, H, 300, 10, THREADS, [150], depth=d, projection=plot.HOLOGRAM, degree=degree, c=c,
                             omp_threads=omp_threads(), states=st)
    assert np.array_equal(want, ref_hist) and {k: wc[k] for k in SAME} == rc
    assert np.array_equal(want_states.view(np.uint32), planar_states(st))


def test_renderer_refuses_a_depth_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(*C_JULIA)
    d = cb.Depth.make("cr", -2.0, 0.5, 5)
    lut = np.full(100, 0x010203, dtype=np.uint32)
    out = np.zeros((5, 64, 64), dtype=">u2")

    def set_depth(r, dd=d):
        return cb.lib.cb_renderer_set_depth(r._h, None if dd is None else C.byref(dd))

    def still_usable(r, shape):
        r.render_passes(1)
        hist = r.read_histogram()
        assert hist.shape == shape and int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0
        assert r.depth() is None and cb.lib.cb_renderer_depth_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID

    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        assert set_depth(r) == INVALID  # a plain renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert set_depth(r) == INVALID  # a channel renderer
        still_usable(r, (2, 64, 64))
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert set_depth(r) == INVALID  # a focused renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_palette(lut)
        assert set_depth(r) == INVALID  # a palette renderer: 3 N planes are out of scope
        still_usable(r, (3, 64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.render_passes(1)
        assert set_depth(r) == INVALID  # after the first pass
        still_usable(r, (64, 64))
    nan, inf = float("nan"), float("inf")
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_julia(C_JULIA)
        fresh = r.read_rng_states().copy()
        assert set_depth(r, None) == INVALID
        for bad in (((nan, 0, 0, 0), 0, 1, 1), ((0, 0, inf, 0), 0, 1, 1), ("cr", nan, 1, 1), ("cr", 0, inf, 1), ("cr", 1, 1, 1),
                    ("cr", 2, 1, 1), ("cr", 0, 1, 0), ("cr", 0, 1, -4), ("cr", 0, 1, 257), ("cr", -1.7e308, 1.7e308, 2)):
            assert set_depth(r, cb.Depth.make(*bad)) == INVALID, bad
        assert r.depth() is None and r.read_histogram().shape == (64, 64)
        r.set_depth(d)
        assert r.depth().as_tuple() == d.as_tuple() and r.julia() == C_JULIA
        assert set_depth(r) == INVALID  # once
        assert cb.lib.cb_renderer_set_palette(r._h, lut.ctypes.data, 100) == INVALID
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED, 9 << 12,
                        cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        hist = r.read_histogram()
        assert hist.shape == (5, 64, 64) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        assert cb.lib.cb_renderer_depth_image(r._h, 1.0, 0, None, None, None) == INVALID
        assert cb.lib.cb_renderer_depth_image(r._h, 1.0, 7, out.ctypes.data, None, None) == INVALID  # no such tone mode
        r.render_passes(1)  # and it renders
        hist = r.read_histogram()
        assert int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0


def test_depth_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads, planes=5)
    buf, counters, states = bufs.out, bufs.counters, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_matrix = (C.c_double * 8)(*([float("nan")] + list(cb.IDENTITY_PROJECTION[1:])))
    c_good = (C.c_double * 2)(*C_JULIA)
    d_good = cb.Depth.make("cr", -2.0, 0.5, 5)
    nan, inf = float("nan"), float("inf")

    def draw(variant=0, c=None, p=good, d=d_good, samples=5, n_threads=threads):
        return cb.lib.cb_draw_buddhabrot_depth(C.byref(dims), buf.data_ptr(), C.byref(it), p, c,
                                               None if d is None else C.byref(d), states.data_ptr(), n_threads, samples,
                                               counters.data_ptr(), variant, None)

    for c in (None, c_good):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=c, d=None) == INVALID
            for bad in (((0, nan, 0, 0), 0, 1, 1), ((0, 0, 0, -inf), 0, 1, 1), ("cr", nan, 1, 1), ("cr", 0, nan, 1),
                        ("cr", -inf, 1, 1), ("cr", 1, 1, 1), ("cr", 2, 1, 1), ("cr", 0, 1, 0), ("cr", 0, 1, 257),
                        ("cr", -1.7e308, 1.7e308, 1)):
                assert draw(base, c=c, d=cb.Depth.make(*bad)) == INVALID, bad
            assert draw(base, c=c, p=None) == INVALID and draw(base, c=c, p=bad_matrix) == INVALID
        power3 = cb.CB_KERNEL_POWER(3)
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_TIMED,
                        cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_DRAIN, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        power3 | cb.CB_KERNEL_FORMULA(2), cb.CB_KERNEL_FORMULA(2) | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        2 << 12, 9 << 12, 6 << 16):
            assert draw(variant, c=c) == INVALID, variant
    for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, inf)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=(C.c_double * 2)(*c)) == INVALID, c
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):  # no threads or no samples: nothing launched, success
        for c in (None, c_good):
            assert draw(base, c=c, samples=0) == 0 and draw(base, c=c, n_threads=0) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)


def host_images(cb, hist, gamma):
    """The header's Image rule on the host: the N planes as one w x N*h image -> ([N, h, w] big-endian u16, max, scale)."""
    n, h, w = hist.shape
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(n * h, w), gamma)
    return gray.reshape(n, h, w).astype(">u2"), mx, scale


@pytest.fixture(scope="module")
def rendered(cb):
    """One renderer with a depth and a few passes in it, and its histogram."""
    dims = cb.FractalDimensions.make(W, H)
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 5))
        r.render_passes(3)
        yield r, r.read_histogram()


@pytest.mark.parametrize("mode", ["CB_TONE_LUT", "CB_TONE_THRESHOLDS"])
@pytest.mark.parametrize("gamma", [1.0, 2.2, -1.0])
def test_depth_image_is_the_tone_map_against_the_common_maximum(cb, rendered, mode, gamma):
    r, hist = rendered
    assert len({int(p.max()) for p in hist}) >= 3  # different maxima: a common one shows
    gray, mx, scale = r.depth_image(gamma, getattr(cb, mode))
    assert gray.shape == (5, H, W) and mx == int(hist.max())
    want = np.array([cb.tone_value(int(v), mx, gamma) for v in hist.reshape(-1)], dtype=np.uint16).reshape(hist.shape)
    assert np.array_equal(gray.astype(np.uint16), want)
    images, want_max, want_scale = host_images(cb, hist, gamma)
    assert (mx, scale) == (want_max, want_scale) and gray.tobytes() == images.tobytes()
    assert int(gray.max()) == 65535 or gamma <= 0


def test_planes_of_a_depth_renderer_tone_map_with_their_own_maximum(cb, rendered):
    r, hist = rendered
    for j in (0, 4):
        gray, mx, _ = r.grayscale_image(1.0, plane=j)
        want, want_max, _ = cb.set_grayscale_pixels(hist[j], 1.0)
        assert mx == want_max == int(hist[j].max()) and np.array_equal(gray.astype(np.uint16), want)
    out = np.zeros((H, W), dtype=">u2")
    assert cb.lib.cb_renderer_grayscale_plane(r._h, 5, 1.0, 0, out.ctypes.data, None, None) == INVALID


# ---- 4. the binary --------------------------------------------------------------------------------------------------------


def parse_pgm_sequence(data):
    """A file of binary 16-bit PGMs back to back -> [(w, h, big-endian u16 [h, w])]."""
    images, at = [], 0
    while at < len(data):
        assert data[at:at + 3] == b"P5\n", data[at:at + 16]
        end = at + 3
        fields = []
        for _ in range(2):
            nl = data.index(b"\n", end)
            fields.append(data[end:nl])
            end = nl + 1
        w, h = (int(v) for v in fields[0].split())
        assert fields[1] == b"65535"
        body = np.frombuffer(data, dtype=">u2", count=w * h, offset=end).reshape(h, w)
        images.append((w, h, body))
        at = end + 2 * w * h
    assert at == len(data)
    return images


def test_cli_depth_images_buffer_and_stats(cb, exe, ref, tmp_path):
    common = ["--depth", "cr:-2:0.5:3", "--plane", "zr,zi", "-w", "64", "-h", "48", "-m", "300", "-c", "20", "--passes", "2"]
    buf, pgm, host_pgm = str(tmp_path / "d.bin"), str(tmp_path / "d.pgm"), str(tmp_path / "host.pgm")
    r = run(exe, *common, "-s", buf, "--stats", "-o", pgm)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saving image." in r.stdout and "Done! Output image saved: %s" % pgm in r.stdout
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"depth": {"row": ["0x0p+0", "0x0p+0", "0x1p+0", "0x0p+0"], "min": "-0x1p+1",
                                              "max": "0x1p-1", "slices": 3}}
    assert run(exe, *common, "--tonemap", "host", "-o", host_pgm).returncode == 0
    with open(pgm, "rb") as f:
        data = f.read()
    with open(host_pgm, "rb") as f:
        assert f.read() == data  # the reference's host loop gives the same file
    images = parse_pgm_sequence(data)
    assert [(w, h) for w, h, _ in images] == [(64, 48)] * 3
    hist = read_state_file(buf, 48, 64, planes=3)  # the header says 3 planes
    want, mx, scale = host_images(cb, hist, 1.0)
    assert "Max value: %d, scale: %f" % (mx, scale) in r.stdout and mx == int(hist.max()) > 0
    for s, (_, _, body) in enumerate(images):
        assert np.array_equal(body, want[s]), s
    assert all(p.any() for p in hist)
    # and the buffer is the restatement's
    ref_hist, rc = plot.draw(ref, 64, 48, 300, 20, 512 * 512, [100], depth=("cr", -2.0, 0.5, 3), omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == rc and np.array_equal(hist, ref_hist)


def test_cli_one_slice_is_an_ordinary_pgm_and_resumes(cb, exe, tmp_path):
    common = ["--depth", "ci:-0.02:0.02", "--julia", "0.3,0.5", "--power", "3", "--kernel", "simple", "-w", "64", "-h",
              "48", "-m", "100", "-c", "5"]
    one_buf, one_side, one_pgm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.pgm")
    assert run(exe, *common, "--passes", "2", "-s", one_buf, "--rng-state", one_side, "-o", one_pgm).returncode == 0
    with open(one_pgm, "rb") as f:
        images = parse_pgm_sequence(f.read())
    assert len(images) == 1 and images[0][:2] == (64, 48)
    read_state_file(one_buf, 48, 64, planes=1)
    buf, side, pgm = str(tmp_path / "two.bin"), str(tmp_path / "two.rng"), str(tmp_path / "two.pgm")
    assert run(exe, *common, "--passes", "1", "-s", buf, "--rng-state", side, "-o", os.devnull).returncode == 0
    r2 = run(exe, *common, "--passes", "1", "-s", buf, "--rng-state", side, "-o", pgm)
    assert r2.returncode == 0 and "Continuing the sample stream after 1 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (pgm, one_pgm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a
    # a buffer of another plane count is refused by the existing check
    r3 = run(exe, "--depth", "ci:-0.02:0.02:2", *common[2:], "--passes", "1", "-s", buf, "-o", os.devnull)
    assert r3.returncode == 1, r3.stdout
