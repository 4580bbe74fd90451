"""The frames render (include/cudabrot_amd.h, "Frames render") on the GPU:

  1. three ways -- the product kernel (cb_debug_last_draw_kernel 22), the lock-step kernel (23), the restatement
     (tests/frames_reference.py: the stack of the CPU's projected renders) -- bit for bit on the F planes, the generator
     states and every counter but skipped_steps;
  2. plane f against the projected and Julia renders on the GPU with P_f: the section's Consequence;
  3. the point queue's edges, product against lock-step;
  4. the most frames there are;
  5. the refusals of the entry point;
  6. the renderer, its refusals and its image;
  7. the binary.

Every comparison is exact.  The shape is plot_harness.DEPTH_SHAPE."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import frames_reference as frames
import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import C_JULIA, DEPTH_SHAPE, INVALID, NOT_INCREMENTS, SAME, SQUARE  # noqa: F401
from plot_harness import exe, omp_threads, planar_states, ref, variant_of  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 22, 23
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE
FAR = (50.0, 51.0, 50.0, 51.0)  # a window no orbit reaches: every plotted coordinate is below 4 * 11 in magnitude


def matrices(m):
    return np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 8)


def frames_launches(cb, variant, mats, c=None, w=W, h=H, box=SQUARE, max_iter=MAX, min_iter=MIN, threads=THREADS,
                    launches=LAUNCHES, states=None):
    """`launches` on fresh generators, or on the given oracle `states` written over them, through
    cb_draw_buddhabrot_frames -> (hist [F, h, w], counters, kernel, states)."""
    mats = matrices(mats)
    bufs = plot_harness.Launches(cb, cb.FractalDimensions.make(w, h, *box), threads, planes=mats.shape[0])
    if states is not None:
        plot_harness.write_states(bufs, states)
    d_frames = bufs.on_device(mats.view(np.uint64), np.uint64)  # kept alive to the read
    out = bufs.launches(cb.draw_buddhabrot_frames, launches, variant, iterations=cb.IterationControl(max_iter, min_iter),
                        d_frames=d_frames.data_ptr(), n_frames=mats.shape[0], julia_c=c).read()
    del d_frames
    return out


def plain_launches(cb, variant, projection, c=None, **kw):
    """The same launches through cb_draw_buddhabrot_projected, or cb_draw_buddhabrot_julia with a c -> hist [h, w]."""
    shape = dict(w=W, h=H, box=SQUARE, max_iter=MAX, min_iter=MIN, threads=THREADS, launches=LAUNCHES)
    shape.update(kw)
    return plot_harness.gpu_launches(cb, shape["w"], shape["h"], shape["box"], shape["max_iter"], shape["min_iter"],
                                     shape["threads"], shape["launches"], variant, c, None, projection)


def both_kernels(cb, mats, *, degree=2, ship=False, formula=0, **kw):
    """Product and lock-step on the same launches, equal on histogram, states and SAME -> the product's (hist, counters)."""
    got = []
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, states = frames_launches(cb, variant_of(cb, base, degree, ship, formula), mats, **kw)
        assert launched == kernel and cnt["status"] == 0 and int(hist.sum()) == cnt["increments"]
        got.append((hist, cnt, states))
    (ph, pc, ps), (lh, lc, ls) = got
    assert np.array_equal(ph, lh) and np.array_equal(ps, ls)
    assert {k: pc[k] for k in SAME} == {k: lc[k] for k in SAME}, (pc, lc)
    assert lc["skipped_steps"] == 0
    return ph, pc


# ---- 1. three ways --------------------------------------------------------------------------------------------------------

CASES = {
    "mandelbrot": dict(),
    "ship": dict(ship=True),
    "power_3": dict(degree=3),
    "tricorn": dict(formula=1),
    "julia": dict(c=C_JULIA),
    "julia_power_3": dict(c=(0.4, 0.0), degree=3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_product_lockstep_and_restatement_agree(cb, ref, oracle, name):
    kw = dict(CASES[name])
    mats, _ = cb.frames_from_sweep(cb.IDENTITY_PROJECTION, ("zi", "cr"), 0.0, 360.0, 5)
    st = oracle.init_states(1337, 0, THREADS)
    want, wc = frames.draw(ref, mats, W, H, MAX, MIN, THREADS, LAUNCHES, states=st, omp_threads=omp_threads(), **kw)
    assert wc["recorded"] > 0 and int(want.sum()) == wc["increments"] > 0 and all(p.any() for p in want)
    mandelbrot = name == "mandelbrot"
    c = kw.pop("c", None)
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, states = frames_launches(cb, variant_of(cb, base, **kw), mats, c)
        print(kernel, cnt)
        assert launched == kernel and cnt["status"] == 0
        assert {k: cnt[k] for k in SAME} == wc, (kernel, cnt, wc)
        assert hist.shape == want.shape and np.array_equal(hist, want), kernel
        assert np.array_equal(states, planar_states(st)), kernel
        level = cb.lib.cb_debug_interior_map_level()
        if mandelbrot and base == cb.CB_KERNEL_DEFAULT:
            assert level >= 1
        else:
            assert level == 0
        if base == cb.CB_KERNEL_SIMPLE:
            assert cnt["skipped_steps"] == 0


# ---- 2. plane f is the projected render with P_f --------------------------------------------------------------------------

UNRELATED = [plot.IDENTITY, plot.HOLOGRAM, plot.plane("zr", "cr")]


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_every_plane_is_the_plain_render_with_its_matrix(cb, c, base):
    hist, cnt, kernel, states = frames_launches(cb, base, UNRELATED, c)
    assert kernel == PRODUCT + base and cnt["status"] == 0 and hist.shape == (3, H, W)
    total = 0
    for f, p in enumerate(UNRELATED):
        plain, pc, plain_kernel, plain_states = plain_launches(cb, base, p, c)
        assert plain_kernel == (12 if c else 8) + base and pc["increments"] > 0
        assert np.array_equal(hist[f], plain), f
        assert {k: cnt[k] for k in NOT_INCREMENTS} == {k: pc[k] for k in NOT_INCREMENTS}
        assert cnt["skipped_steps"] == pc["skipped_steps"]  # the same early-outs, the same map
        assert np.array_equal(states, plain_states)
        total += pc["increments"]
    assert cnt["increments"] == total


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_one_frame_is_the_plain_render_in_everything(cb, c, base):
    hist, cnt, _, states = frames_launches(cb, base, [plot.HOLOGRAM], c)
    plain, pc, _, plain_states = plain_launches(cb, base, plot.HOLOGRAM, c)
    assert hist.shape == (1, H, W) and pc["increments"] > 0 and np.array_equal(hist[0], plain)
    assert {k: cnt[k] for k in SAME + ("skipped_steps", "status")} == {k: pc[k] for k in SAME + ("skipped_steps", "status")}
    assert np.array_equal(states, plain_states)


# ---- 3. the point queue's edges -------------------------------------------------------------------------------------------

TWO = [plot.HOLOGRAM, plot.plane("zr", "cr")]


@pytest.mark.parametrize("launches", [(1,), (2, 1)])
@pytest.mark.parametrize("threads", [1, 63, 64, 65, 70, 257, THREADS])
def test_queue_with_few_lanes_ragged_waves_and_short_launches(cb, threads, launches):
    hist, cnt = both_kernels(cb, TWO, threads=threads, launches=launches)
    assert cnt["samples"] == threads * sum(launches)
    if threads == THREADS:
        assert cnt["increments"] > 0


@pytest.mark.parametrize("threads", [1, 63, 64, 65, 70, 257])
def test_queue_with_few_lanes_and_many_samples_under_a_fixed_c(cb, threads):
    hist, cnt = both_kernels(cb, TWO, threads=threads, launches=(60,), c=C_JULIA)
    assert cnt["samples"] == threads * 60 and (cnt["increments"] > 0 or threads == 1)


@pytest.mark.parametrize("max_iter, min_iter", [(1, 0), (13, 0), (0, 0)])
@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_queue_with_one_point_orbits_orbits_past_a_round_and_none(cb, c, max_iter, min_iter):
    hist, cnt = both_kernels(cb, TWO, c=c, max_iter=max_iter, min_iter=min_iter)
    if max_iter == 0:
        assert cnt["increments"] == 0 and not hist.any() and cnt["recorded"] == 0 and cnt["samples"] == THREADS * 54
    else:
        assert cnt["recorded"] > 0 and cnt["increments"] > 0
        if max_iter == 1:
            assert cnt["replay_steps"] == cnt["recorded"]  # one-point orbits
        else:
            assert cnt["replay_steps"] > 12 * 10  # some orbits run past the first round


@pytest.mark.parametrize("c", [None, C_JULIA], ids=["projected", "julia"])
def test_a_canvas_no_orbit_reaches_changes_increments_alone(cb, c):
    hist, cnt = both_kernels(cb, TWO, c=c, box=FAR)
    seen, sc = both_kernels(cb, TWO, c=c)
    assert cnt["increments"] == 0 and not hist.any() and sc["increments"] > 0
    assert {k: cnt[k] for k in NOT_INCREMENTS} == {k: sc[k] for k in NOT_INCREMENTS}
    assert cnt["skipped_steps"] == sc["skipped_steps"]


@pytest.mark.parametrize("n", [2, 64])
def test_queue_with_few_and_many_frames(cb, n):
    mats, _ = cb.frames_from_sweep(plot.HOLOGRAM, ("zi", "cr"), 0.0, 90.0, n)
    hist, cnt = both_kernels(cb, mats)
    assert hist.shape == (n, H, W) and all(p.any() for p in hist)
    plain, pc, _, _ = plain_launches(cb, 0, mats[n - 1])
    assert np.array_equal(hist[n - 1], plain)


# ---- 4. the most frames there are -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
def test_256_identical_matrices_give_256_identical_planes(cb, base):
    mats = np.tile(matrices(plot.HOLOGRAM), (256, 1))
    hist, cnt, kernel, _ = frames_launches(cb, base, mats, w=16, h=8, threads=256, launches=(5,))
    assert kernel == PRODUCT + base and cnt["status"] == 0 and hist.shape == (256, 8, 16)
    assert hist[0].any() and (hist == hist[0]).all()
    assert cnt["increments"] == 256 * int(hist[0].sum())
    plain, _, _, _ = plain_launches(cb, base, plot.HOLOGRAM, w=16, h=8, threads=256, launches=(5,))
    assert np.array_equal(hist[255], plain)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------


def test_frames_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    tall = cb.FractalDimensions.make(1, 8388609)  # 256 * h is one row above INT_MAX
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads, planes=3)
    buf, counters, states = bufs.out, bufs.counters, bufs.states
    good = bufs.on_device(np.tile(matrices(plot.IDENTITY), (256, 1)).view(np.uint64), np.uint64)
    bad = np.tile(matrices(plot.IDENTITY), (3, 1))
    bad[2, 5] = float("nan")
    bad = bufs.on_device(bad.view(np.uint64), np.uint64)
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    c_good = (C.c_double * 2)(*C_JULIA)

    def draw(variant=0, c=None, d_frames=good, n=3, d=dims, samples=5):
        return cb.lib.cb_draw_buddhabrot_frames(C.byref(d), buf.data_ptr(), C.byref(it),
                                                None if d_frames is None else d_frames.data_ptr(), n, c, states.data_ptr(),
                                                threads, samples, counters.data_ptr(), variant, None)

    power3 = cb.CB_KERNEL_POWER(3)
    for c in (None, c_good):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c, n=0) == INVALID and draw(base, c, n=257) == INVALID and draw(base, c, n=-1) == INVALID
            assert draw(base, c, d_frames=None) == INVALID
            assert draw(base, c, d_frames=bad) == INVALID  # looked at in a host copy of the device's matrices
            assert draw(base, c, n=256, d=tall) == INVALID
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN,
                        cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        power3 | cb.CB_KERNEL_FORMULA(2), cb.CB_KERNEL_FORMULA(2) | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                        2 << 12, 9 << 12, 6 << 16):
            assert draw(variant, c) == INVALID, variant
    for c in ((2.5, 0.0), (float("nan"), 0.0)):
        assert draw(0, (C.c_double * 2)(*c)) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):  # no samples: nothing launched, success
        assert draw(base, samples=0) == 0
    assert draw(0, d_frames=bad, n=2) == 0  # the NaN lies in the third matrix: two are fine
    torch.cuda.synchronize()
    assert int(buf.sum()) == bufs.read_counters()["increments"] > 0


# ---- 6. the renderer ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("kind", ["projected", "julia_power_3"])
def test_renderer_passes_are_the_entry_points_launches(cb, base, kind):
    c, degree = ((0.4, 0.0), 3) if kind == "julia_power_3" else (None, 2)
    variant = variant_of(cb, base, degree)
    mats, _ = cb.frames_from_sweep(plot.HOLOGRAM, ("zi", "cr"), 10.0, 100.0, 4)
    with cb.Renderer(cb.FractalDimensions.make(W, H), cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        if c is None:
            r.set_projection(plot.HOLOGRAM)
        else:
            r.set_julia(c, plot.HOLOGRAM)
        assert r.frames() is None and cb.lib.cb_renderer_frames(r._h, None) == 0
        r.set_frames(mats)
        assert np.array_equal(r.frames(), mats) and cb.lib.cb_renderer_frames(r._h, None) == 4
        r.prepare(variant)
        r.render_passes(1, variant)
        r.render_passes(2, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT + base
        hist, cnt, states = r.read_histogram(), r.read_counters().as_dict(), r.read_rng_states().copy()
        with pytest.raises(ValueError):
            r.write_histogram(hist[0])
        r.write_histogram(hist)
        assert np.array_equal(r.read_histogram(), hist)
    per = cb.CB_SAMPLES_PER_THREAD
    want, wc, _, want_states = frames_launches(cb, variant, mats, c, launches=(per, 2 * per))
    assert hist.shape == (4, H, W) and np.array_equal(hist, want) and wc["increments"] > 0
    assert {k: cnt[k] for k in SAME + ("skipped_steps", "status")} == {k: wc[k] for k in SAME + ("skipped_steps", "status")}
    assert np.array_equal(states.view(np.uint32), want_states)


def test_renderer_refuses_frames_where_they_are_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(*C_JULIA)
    mats, _ = cb.frames_from_sweep(cb.IDENTITY_PROJECTION, ("zi", "cr"), 0.0, 90.0, 3)
    d = cb.Depth.make("cr", -2.0, 0.5, 5)
    lut = np.full(100, 0x010203, dtype=np.uint32)
    out = np.zeros((5, 64, 64), dtype=">u2")

    def set_frames(r, m=mats, n=None):
        return cb.lib.cb_renderer_set_frames(r._h, None if m is None else m.ctypes.data, len(m) if n is None else n)

    def still_usable(r, shape):
        r.render_passes(1)
        hist = r.read_histogram()
        assert hist.shape == shape and int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0
        assert r.frames() is None and cb.lib.cb_renderer_frames_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID

    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        assert set_frames(r) == INVALID  # a plain renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert set_frames(r) == INVALID  # a channel renderer
        still_usable(r, (2, 64, 64))
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert set_frames(r) == INVALID  # a focused renderer
        still_usable(r, (64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_palette(lut)
        assert set_frames(r) == INVALID  # a palette renderer
        still_usable(r, (3, 64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(d)
        assert set_frames(r) == INVALID  # a renderer with a depth
        still_usable(r, (5, 64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth_palette(d, lut[:5])
        assert set_frames(r) == INVALID  # a renderer with a depth palette
        still_usable(r, (3, 64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.render_passes(1)
        assert set_frames(r) == INVALID  # after the first pass
        still_usable(r, (64, 64))
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_julia(C_JULIA)
        fresh = r.read_rng_states().copy()
        nan_mats = mats.copy()
        nan_mats[1, 3] = float("inf")
        assert set_frames(r, None, 3) == INVALID and set_frames(r, mats, 0) == INVALID and set_frames(r, mats, 257) == INVALID
        assert set_frames(r, nan_mats) == INVALID
        assert r.frames() is None and r.read_histogram().shape == (64, 64)
        r.set_frames(mats)
        assert np.array_equal(r.frames(), mats) and r.julia() == C_JULIA
        assert set_frames(r) == INVALID  # once
        assert cb.lib.cb_renderer_set_palette(r._h, lut.ctypes.data, 100) == INVALID
        assert cb.lib.cb_renderer_set_depth(r._h, C.byref(d)) == INVALID
        assert cb.lib.cb_renderer_set_depth_palette(r._h, C.byref(d), lut.ctypes.data, 5) == INVALID
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        assert r.depth() is None and r.depth_palette() is None and r.palette() is None
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED, 9 << 12,
                        cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        hist = r.read_histogram()
        assert hist.shape == (3, 64, 64) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        assert cb.lib.cb_renderer_frames_image(r._h, 1.0, 0, None, None, None) == INVALID
        assert cb.lib.cb_renderer_depth_image(r._h, 1.0, 0, out.ctypes.data, None, None) == INVALID
        r.render_passes(1)  # and it renders
        hist = r.read_histogram()
        assert int(hist.sum()) == r.read_counters().as_dict()["increments"] > 0


def host_images(cb, hist, gamma):
    """The header's Image rule on the host: the F planes as one w x F*h image -> ([F, h, w] big-endian u16, max, scale)."""
    n, h, w = hist.shape
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(n * h, w), gamma)
    return gray.reshape(n, h, w).astype(">u2"), mx, scale


@pytest.fixture(scope="module")
def rendered(cb):
    """One renderer with frames and a few passes in it, and its histogram."""
    mats, _ = cb.frames_from_sweep(cb.IDENTITY_PROJECTION, ("zi", "cr"), 0.0, 90.0, 5)
    with cb.Renderer(cb.FractalDimensions.make(W, H), cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_frames(mats)
        r.render_passes(3)
        yield r, r.read_histogram()


@pytest.mark.parametrize("mode", ["CB_TONE_LUT", "CB_TONE_THRESHOLDS"])
@pytest.mark.parametrize("gamma", [1.0, 2.2, -1.0])
def test_frames_image_is_the_tone_map_against_the_common_maximum(cb, rendered, mode, gamma):
    r, hist = rendered
    assert len({int(p.max()) for p in hist}) >= 3  # different maxima: a common one shows
    gray, mx, scale = r.frames_image(gamma, getattr(cb, mode))
    assert gray.shape == (5, H, W) and mx == int(hist.max())
    want = np.array([cb.tone_value(int(v), mx, gamma) for v in hist.reshape(-1)], dtype=np.uint16).reshape(hist.shape)
    assert np.array_equal(gray.astype(np.uint16), want)
    images, want_max, want_scale = host_images(cb, hist, gamma)  # what --tonemap host does
    assert (mx, scale) == (want_max, want_scale) and gray.tobytes() == images.tobytes()
    assert int(gray.max()) == 65535 or gamma <= 0


def test_planes_of_a_frames_renderer_tone_map_with_their_own_maximum(cb, rendered):
    r, hist = rendered
    for j in (0, 4):
        gray, mx, _ = r.grayscale_image(1.0, plane=j)
        want, want_max, _ = cb.set_grayscale_pixels(hist[j], 1.0)
        assert mx == want_max == int(hist[j].max()) and np.array_equal(gray.astype(np.uint16), want)
    out = np.zeros((H, W), dtype=">u2")
    assert cb.lib.cb_renderer_grayscale_plane(r._h, 5, 1.0, 0, out.ctypes.data, None, None) == INVALID


# ---- 7. the binary --------------------------------------------------------------------------------------------------------


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
        images.append((w, h, np.frombuffer(data, dtype=">u2", count=w * h, offset=end).reshape(h, w)))
        at = end + 2 * w * h
    assert at == len(data)
    return images


SHAPE = ["-w", "64", "-h", "48", "-m", "300", "-c", "20"]


def test_cli_sweep_planes_are_the_rotated_runs_and_the_images_share_one_exposure(cb, exe, tmp_path):
    buf, pgm, host_pgm = str(tmp_path / "s.bin"), str(tmp_path / "s.pgm"), str(tmp_path / "host.pgm")
    r = run(exe, "--sweep", "zi,cr:0:360:4", *SHAPE, "--passes", "2", "-s", buf, "--stats", "-o", pgm)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saving image." in r.stdout and "Done! Output image saved: %s" % pgm in r.stdout
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    sweep = json.loads(lines[1])["sweep"]
    assert sweep["axes"] == ["zi", "cr"] and sweep["frames"] == 4
    assert float.fromhex(sweep["from"]) == 0.0 and float.fromhex(sweep["to"]) == 360.0
    assert [float.fromhex(a) for a in sweep["angles"]] == [0.0, 90.0, 180.0, 270.0]
    stats = json.loads(lines[-1])
    hist = read_state_file(buf, 48, 64, planes=4)  # the header says 4 planes
    assert stats["status"] == 0 and stats["increments"] == int(hist.sum()) and all(p.any() for p in hist)
    recorded = None
    for f, angle in enumerate(sweep["angles"]):  # --rotate X,Y:<a_f> reproduces frame f
        one = str(tmp_path / ("r%d.bin" % f))
        rr = run(exe, "--rotate", "zi,cr:" + angle, *SHAPE, "--passes", "2", "-s", one, "--stats", "-o", os.devnull)
        assert rr.returncode == 0, rr.stdout + rr.stderr
        assert np.array_equal(read_state_file(one, 48, 64), hist[f]), f
        single = json.loads(rr.stderr.strip().split("\n")[-1])
        assert {k: single[k] for k in NOT_INCREMENTS} == {k: stats[k] for k in NOT_INCREMENTS}
        recorded = single["recorded"]
    assert recorded > 0
    # the images: four PGMs, the brightest sample in exactly the frame that holds the maximum
    assert run(exe, "--sweep", "zi,cr:0:360:4", *SHAPE, "--passes", "2", "--tonemap", "host", "-o", host_pgm).returncode == 0
    with open(pgm, "rb") as f:
        data = f.read()
    with open(host_pgm, "rb") as f:
        assert f.read() == data
    images = parse_pgm_sequence(data)
    assert [(w, h) for w, h, _ in images] == [(64, 48)] * 4
    want, mx, scale = host_images(cb, hist, 1.0)
    assert "Max value: %d, scale: %f" % (mx, scale) in r.stdout and mx == int(hist.max()) > 0
    for f, (_, _, body) in enumerate(images):
        assert np.array_equal(body, want[f]), f
        assert (int(body.max()) == 65535) == (int(hist[f].max()) == mx), f


def test_cli_sweep_resumes_and_takes_julia_and_a_formula(exe, tmp_path):
    common = ["--sweep", "zr,ci:5:50:3", "--julia", "-0.8,0.156", "--formula", "celtic", "--plane", "zi,zr", *SHAPE]
    one_buf, one_side, one_pgm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.pgm")
    r = run(exe, *common, "--passes", "3", "-s", one_buf, "--rng-state", one_side, "-o", one_pgm, "--stats")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(v) for v in r.stderr.strip().split("\n")]
    assert [float.fromhex(v) for v in lines[0]["projection"]] == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]  # the base
    assert any("formula" in v for v in lines) and any("julia" in v for v in lines)
    sweep = [v for v in lines if "sweep" in v][0]["sweep"]
    assert [float.fromhex(a) for a in sweep["angles"]] == [5.0, 5.0 + (45.0 * 1.0) / 3.0, 5.0 + (45.0 * 2.0) / 3.0]
    hist = read_state_file(one_buf, 48, 64, planes=3)
    assert lines[-1]["status"] == 0 and lines[-1]["increments"] == int(hist.sum()) > 0
    buf, side, pgm = str(tmp_path / "two.bin"), str(tmp_path / "two.rng"), str(tmp_path / "two.pgm")
    assert run(exe, *common, "--passes", "2", "-s", buf, "--rng-state", side, "-o", os.devnull).returncode == 0
    r2 = run(exe, *common, "--passes", "1", "-s", buf, "--rng-state", side, "-o", pgm)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (pgm, one_pgm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a
    # the lock-step kernel through the binary gives the same buffer
    simple = str(tmp_path / "simple.bin")
    assert run(exe, *common, "--kernel", "simple", "--passes", "3", "-s", simple, "-o", os.devnull).returncode == 0
    assert np.array_equal(read_state_file(simple, 48, 64, planes=3), hist)
