"""The Phoenix render (include/cudabrot_amd.h, "Phoenix render") on the GPU:

  1. three ways -- the product kernel (cb_debug_last_draw_kernel 24), the lock-step kernel (25), the CPU restatement
     (tests/phoenix_reference.c) -- bit for bit on histogram, generator states and every counter but skipped_steps;
  2. the inputs reach the paths: accepted orbits and exact cycles occur, and a z-only cycle test would differ;
  3. the cycle test compares the whole state: the product kernel's skipped_steps is the restatement's discount under the
     state rule, to the step, and not the z-only rule's;
  4. p = 0 is the Julia render (kernels 12 and 13) and the projected render without rejection;
  5. the edges of the grid, of the launches, of the iteration control and of the canvas;
  6. everything the ABI refuses;
  7. the renderer;
  8. the binary.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import phoenix_reference as phoenix
import plot_harness
import plot_reference as plot
from conftest import read_state_file
from phoenix_harness import phoenix_launches, restated, shape_of, three_ways  # noqa: F401
from plot_harness import DEPTH_SHAPE, INVALID, SAME, SQUARE, exe, omp_threads, planar_states, ref  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 24, 25
W, H, MAX, MIN, THREADS, LAUNCHES = DEPTH_SHAPE
CASES = {
    "sampled": dict(p=(-0.5, 0.0)),
    "sampled_hologram": dict(p=(0.3, -0.4), projection=plot.HOLOGRAM, w=333, h=77, box=(-1.5, 0.7, -0.9, 1.1)),
    "julia": dict(c=(-0.8, 0.156), p=(0.25, 0.0)),
    "phoenix_julia_zr_cr": dict(c=(0.56667, 0.0), p=(-0.5, 0.0), projection=plot.ZR_CR),
}


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return phoenix.load(tmp_path_factory.mktemp("phoenix_ref"))


# ---- 1 - 3. three ways, on inputs that reach the paths, with the whole state compared ----------------------------------


@pytest.fixture(scope="module")
def cases(cb, pref, oracle):
    """Every case three ways, once for the module."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = three_ways(cb, pref, oracle, **CASES[name])
        return done[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_three_ways(cases, name):
    want, wc, extra, product = cases(name)
    assert wc["recorded"] > 0 and wc["increments"] > 0 and want.any()
    if name == "sampled_hologram":  # the cropped canvas: points on it and off it
        assert wc["increments"] < wc["replay_steps"]


@pytest.mark.parametrize("name", ["sampled", "julia"])
def test_the_inputs_reach_accepted_orbits_and_exact_cycles(cases, name):
    _, wc, extra, _ = cases(name)
    assert wc["recorded"] > 0 and wc["never_escaped"] > 0 and extra["skipped_state"] > 0 and extra["cycles_state"] > 0
    if name == "sampled":
        assert extra["skipped_state"] != extra["skipped_z_only"]


def test_the_cycle_test_compares_the_whole_state(cases):
    """z_k == z_saved with another y proves nothing about z_{k+1}: a scheduler that compared z alone would retire some
    samples earlier, and its discount would be the z-only rule's.  The product kernel's is the state rule's, to the step."""
    _, _, extra, product = cases("sampled")
    assert extra["cycles_z_only"] >= extra["cycles_state"] and extra["skipped_z_only"] > extra["skipped_state"]
    assert product["skipped_steps"] == extra["skipped_state"] != extra["skipped_z_only"]


# ---- 4. p = 0 --------------------------------------------------------------------------------------------------------------


def test_p_zero_with_a_fixed_c_is_the_julia_render(cb):
    c = (-0.8, 0.156)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        hist, cnt, kernel, states = phoenix_launches(cb, base, p=(0.0, 0.0), c=c)
        assert kernel == (LOCKSTEP if base else PRODUCT) and cnt["status"] == 0 and cnt["recorded"] > 0
        for julia_base, julia_kernel in ((cb.CB_KERNEL_DEFAULT, 12), (cb.CB_KERNEL_SIMPLE, 13)):
            jh, jc, launched, js = plot_harness.gpu_launches(cb, W, H, SQUARE, MAX, MIN, THREADS, LAUNCHES, julia_base, c)
            assert launched == julia_kernel
            assert np.array_equal(hist, jh) and np.array_equal(states, js)
            assert {k: cnt[k] for k in SAME} == {k: jc[k] for k in SAME}


def test_p_zero_with_a_sampled_c_is_the_projected_render_without_rejection(cb, ref, oracle):  # noqa: F811
    st = oracle.init_states(1337, 0, THREADS)
    want, wc = plot.draw(ref, W, H, MAX, MIN, THREADS, LAUNCHES, reject=False, states=st, omp_threads=omp_threads())
    assert wc["rejected"] == 0 and wc["recorded"] > 0 and wc["never_escaped"] > 0
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        hist, cnt, _, states = phoenix_launches(cb, base, p=(0.0, 0.0))
        assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == wc
        assert np.array_equal(hist, want) and np.array_equal(states, planar_states(st))


# ---- 5. edges --------------------------------------------------------------------------------------------------------------

EDGES = {
    "threads_1": dict(threads=1, launches=(40,)),
    "threads_63": dict(threads=63),
    "threads_64": dict(threads=64),
    "threads_65": dict(threads=65),
    "threads_257": dict(threads=257),
    "one_sample": dict(launches=(1,)),
    "two_then_one": dict(launches=(2, 1)),
    "max_0": dict(max_iter=0, min_iter=0),
    "max_1": dict(max_iter=1, min_iter=0),
    "max_13": dict(max_iter=13, min_iter=2),
    "max_60": dict(max_iter=60, min_iter=5),
    "max_61": dict(max_iter=61, min_iter=5),
    "max_120": dict(max_iter=120, min_iter=5),
    "max_121": dict(max_iter=121, min_iter=5),
    "min_is_max": dict(max_iter=100, min_iter=100),
    "min_above_max": dict(max_iter=100, min_iter=150),
    "canvas_nothing_reaches": dict(box=(10.0, 11.0, 10.0, 11.0)),
}


@pytest.mark.parametrize("source", ["sampled", "fixed"])
@pytest.mark.parametrize("name", list(EDGES))
def test_edges(cb, pref, oracle, name, source):
    kw = dict(p=(-0.5, 0.0), **EDGES[name])
    if source == "fixed":
        kw.update(c=(0.56667, 0.0))
    want, wc, extra, product = three_ways(cb, pref, oracle, **kw)
    if name == "max_0":
        assert wc["never_escaped"] == wc["samples"] and wc["iterate_steps"] == 0 and wc["increments"] == 0
    elif name == "max_1":  # only k == 0 is accepted: one replayed point, z_1
        assert wc["replay_steps"] == wc["recorded"]
    elif name in ("min_is_max", "min_above_max"):
        assert wc["recorded"] == 0 and wc["increments"] == 0 and not want.any() and wc["too_fast"] > 0
    elif name == "canvas_nothing_reaches":
        assert wc["recorded"] > 0 and wc["replay_steps"] > 0 and wc["increments"] == 0 and not want.any()
    if name in ("max_0", "max_1", "max_13", "max_60", "max_61", "max_120"):
        assert product["skipped_steps"] == 0  # the first comparison is at k = 120 < max


def test_consecutive_launches_equal_one_launch_of_the_sum(cb):
    for c in (None, (-0.8, 0.156)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            a = phoenix_launches(cb, base, p=(0.3, -0.4), c=c, launches=(3, 50, 1))
            b = phoenix_launches(cb, base, p=(0.3, -0.4), c=c, launches=(54,))
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
            assert {k: a[1][k] for k in SAME + ("skipped_steps",)} == {k: b[1][k] for k in SAME + ("skipped_steps",)}
            assert a[1]["recorded"] > 0


# ---- 6. what the ABI refuses ---------------------------------------------------------------------------------------------


def test_phoenix_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads)
    buf, states, counters = bufs.out, bufs.states, bufs.counters
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    p_good = (C.c_double * 2)(-0.5, 0.0)
    c_good = (C.c_double * 2)(-0.8, 0.156)
    d, b, i, s = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr()

    def draw(variant=0, p=p_good, c=None, m=good, samples=5):
        return cb.lib.cb_draw_buddhabrot_phoenix(d, b, i, m, c, p, s, threads, samples, counters.data_ptr(), variant, None)

    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf, 2.0000001, -2.0000001):
        for p in ((bad, 0.0), (0.0, bad)):
            for c in (None, c_good):
                for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
                    assert draw(base, (C.c_double * 2)(*p), c) == INVALID, p
    assert draw(p=None) == INVALID
    power3, tricorn = cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA(1)
    flags = [cb.CB_KERNEL_FLAG_BURNING_SHIP, cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, power3, tricorn,
             cb.CB_KERNEL_POWER(8), cb.CB_KERNEL_FORMULA(5), power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP, 2 << 12, 9 << 12, 6 << 16]
    for flag in flags:
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            for c in (None, c_good):
                assert draw(base | flag, c=c) == INVALID, (base, flag)
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE):
        assert draw(variant) == INVALID, variant
    for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, inf)):
        assert draw(c=(C.c_double * 2)(*c)) == INVALID, c
    for j in range(8):
        for bad in (nan, inf):
            m = list(cb.IDENTITY_PROJECTION)
            m[j] = bad
            assert draw(m=(C.c_double * 8)(*m)) == INVALID
    assert draw(m=None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success; the bounds of p are allowed
    assert draw(samples=0) == 0
    assert cb.lib.cb_draw_buddhabrot_phoenix(d, b, i, good, None, p_good, s, 0, 5, counters.data_ptr(), 0, None) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)
    assert draw(p=(C.c_double * 2)(2.0, -2.0)) == 0 and draw(1, p=(C.c_double * 2)(-2.0, 2.0), c=c_good) == 0
    torch.cuda.synchronize()
    assert bufs.read_counters()["samples"] == 2 * 5 * threads


# ---- 7. the renderer -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", ["sampled_hologram", "phoenix_julia_zr_cr"])
def test_renderer_against_the_entry_point_on_identical_passes(cb, base, name):
    kw = shape_of(CASES[name])
    kw.update(launches=(50, 100))  # one pass, then two fused: the same samples per generator
    want, wc, kernel, states = phoenix_launches(cb, base, **kw)
    dims = cb.FractalDimensions.make(kw["w"], kw["h"], *kw["box"])
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        if kw["c"] is None:
            r.set_projection(kw["projection"])
        else:
            r.set_julia(kw["c"], kw["projection"])
        assert r.phoenix() is None
        r.set_phoenix(kw["p"])
        assert r.phoenix() == tuple(kw["p"])
        assert r.julia() == (None if kw["c"] is None else tuple(kw["c"]))
        r.prepare(base)  # must not fail
        r.render_passes(1, base)
        r.finish()
        r.render_passes(2, base)
        assert cb.lib.cb_debug_last_draw_kernel() == kernel == PRODUCT + base
        assert cb.lib.cb_renderer_interior_map_level(r._h) == 0
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        after = r.read_rng_states().view(np.uint32)
        assert hist.shape == (kw["h"], kw["w"])
        assert cnt["status"] == 0 and {k: cnt[k] for k in SAME + ("skipped_steps",)} == {
            k: wc[k] for k in SAME + ("skipped_steps",)}
        assert wc["recorded"] > 0 and np.array_equal(hist, want) and np.array_equal(after, states)
        # the image is the one plane's: the reference's tone map of the histogram
        for gamma in (1.0, 2.2):
            gray, mx, scale = r.grayscale_image(gamma)
            want_gray, want_max, want_scale = cb.set_grayscale_pixels(hist, gamma)
            assert mx == want_max == int(hist.max()) > 0 and scale == want_scale
            assert np.array_equal(gray.astype(np.uint16), want_gray)
        # the buffer and the generators go out and come back as for a Julia renderer
        r.write_histogram(hist)
        r.write_rng_states(r.read_rng_states())
        assert np.array_equal(r.read_histogram(), hist)


def test_renderer_refuses_phoenix_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    p_good = (C.c_double * 2)(-0.5, 0.0)
    c_good = (C.c_double * 2)(-0.8, 0.156)
    out = (C.c_double * 2)(7.0, 7.0)

    def set_phoenix(r, p=p_good):
        return cb.lib.cb_renderer_set_phoenix(r._h, p)

    # the order is projection, then julia, then phoenix: before either it is refused, and afterwards they are
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        assert set_phoenix(r) == INVALID  # a plain renderer
        assert cb.lib.cb_renderer_phoenix(r._h, out) == 0 and list(out) == [7.0, 7.0]
        r.set_projection(cb.IDENTITY_PROJECTION)  # and it is still a renderer that can become one
        assert set_phoenix(r) == 0 and r.phoenix() == (-0.5, 0.0)
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert set_phoenix(r) == INVALID and r.phoenix() is None  # a channel renderer
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert set_phoenix(r) == INVALID  # a focused renderer
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_palette(plot.demo_table(100))
        assert set_phoenix(r) == INVALID  # a palette renderer
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 4))
        assert set_phoenix(r) == INVALID  # a depth
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_julia((-0.8, 0.156))
        r.set_depth_palette(("cr", -2.0, 0.5, 4), plot.demo_table(4))
        assert set_phoenix(r) == INVALID  # a depth palette
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_frames(np.array([cb.IDENTITY_PROJECTION] * 2))
        assert set_phoenix(r) == INVALID  # frames
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.render_passes(1)
        assert set_phoenix(r) == INVALID and r.phoenix() is None  # after the first pass
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_julia((-0.8, 0.156))
        fresh = r.read_rng_states().copy()
        nan, inf = float("nan"), float("inf")
        for p in ((2.0000001, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
            assert set_phoenix(r, (C.c_double * 2)(*p)) == INVALID
        assert set_phoenix(r, None) == INVALID and r.phoenix() is None
        assert set_phoenix(r) == 0 and r.phoenix() == (-0.5, 0.0) and r.julia() == (-0.8, 0.156)
        assert set_phoenix(r) == INVALID  # once
        # afterwards the other setters are refused, as after cb_renderer_set_depth
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        for attempt in (lambda: r.set_palette(plot.demo_table(100)), lambda: r.set_depth(("cr", -2.0, 0.5, 4)),
                        lambda: r.set_depth_palette(("cr", -2.0, 0.5, 4), plot.demo_table(4)),
                        lambda: r.set_frames(np.array([cb.IDENTITY_PROJECTION] * 2))):
            with pytest.raises(cb.CudabrotError) as e:
                attempt()
            assert e.value.code == INVALID
        # render_passes and prepare take the two base variants without flag bits
        for variant in (cb.CB_KERNEL_FLAG_BURNING_SHIP, cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA(1),
                        cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID, variant
            assert cb.lib.cb_renderer_prepare(r._h, variant) == INVALID, variant
        hist = r.read_histogram()
        assert hist.shape == (64, 64) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        r.render_passes(1)  # and it renders
        assert int(r.read_histogram().sum()) == r.read_counters().as_dict()["increments"] > 0
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT


# ---- 8. the binary -------------------------------------------------------------------------------------------------------

CLI_W, CLI_H, CLI_MAX, CLI_MIN = 64, 48, 200, 10


def api_render(cb, passes, base=0, c=None, p=(-0.5, 0.0), projection=plot.IDENTITY):
    """What the binary's run is: a renderer of its default threads and seed -> (hist, counters)."""
    dims = cb.FractalDimensions.make(CLI_W, CLI_H)
    with cb.Renderer(dims, cb.IterationControl(CLI_MAX, CLI_MIN), device=0) as r:
        if c is None:
            r.set_projection(projection)
        else:
            r.set_julia(c, projection)
        r.set_phoenix(p)
        r.render_passes(passes, base)
        return r.read_histogram(), r.read_counters().as_dict()


def test_cli_phoenix_equals_the_api_resumes_and_selects_its_kernels(cb, exe, tmp_path):
    common = ["--phoenix", "-0.5,0", "-w", str(CLI_W), "-h", str(CLI_H), "-m", str(CLI_MAX), "-c", str(CLI_MIN), "-o",
              os.devnull]
    want, wc = api_render(cb, 3)
    assert wc["recorded"] > 0 and wc["skipped_steps"] > 0
    one_buf, one_side = str(tmp_path / "one.bin"), str(tmp_path / "one.rng")
    r = run(exe, "--passes", "3", "-s", one_buf, "--rng-state", one_side, "--stats", *common)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert [float.fromhex(v) for v in json.loads(lines[1])["phoenix"]] == [-0.5, 0.0]
    stats = json.loads(lines[-1])
    keys = SAME + ("skipped_steps",)
    assert stats["status"] == 0 and {k: stats[k] for k in keys} == {k: wc[k] for k in keys}
    assert np.array_equal(read_state_file(one_buf, CLI_H, CLI_W), want)
    # two passes, the two files written, then one more pass on them: the same run
    buf, side = str(tmp_path / "two.bin"), str(tmp_path / "two.rng")
    assert run(exe, "--passes", "2", "-s", buf, "--rng-state", side, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        assert a.read() == b.read()
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()
    # the raw format is the one plane's
    raw = str(tmp_path / "raw.bin")
    assert run(exe, "--passes", "3", "-s", raw, "--state-format", "raw", *common).returncode == 0
    assert np.array_equal(np.fromfile(raw, dtype=np.uint32).reshape(CLI_H, CLI_W), want)
    # --kernel simple is the lock-step kernel (25): the same buffer and counters, and nothing skipped; the default is the
    # product kernel (24), whose early-out shows in skipped_steps
    simple = str(tmp_path / "simple.bin")
    r3 = run(exe, "--kernel", "simple", "--passes", "3", "-s", simple, "--stats", *common)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    stats3 = json.loads(r3.stderr.strip().split("\n")[-1])
    assert {k: stats3[k] for k in SAME} == {k: wc[k] for k in SAME} and stats3["skipped_steps"] == 0 < stats["skipped_steps"]
    assert np.array_equal(read_state_file(simple, CLI_H, CLI_W), want)
    lock, lc = api_render(cb, 3, base=cb.CB_KERNEL_SIMPLE)
    assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP and lc["skipped_steps"] == 0 and np.array_equal(lock, want)


def test_cli_phoenix_julia_on_another_plane(cb, exe, tmp_path):
    buf = str(tmp_path / "pj.bin")
    r = run(exe, "--julia", "0.56667,0", "--phoenix", "-0.5,0", "--plane", "zr,cr", "--passes", "1", "-w", str(CLI_W), "-h",
            str(CLI_H), "-m", str(CLI_MAX), "-c", str(CLI_MIN), "-s", buf, "--stats", "-o", os.devnull)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert "julia" in json.loads(lines[1]) and "phoenix" in json.loads(lines[2])
    want, wc = api_render(cb, 1, c=(0.56667, 0.0), projection=plot.ZR_CR)
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == {k: wc[k] for k in SAME}
    assert wc["recorded"] > 0 and np.array_equal(read_state_file(buf, CLI_H, CLI_W), want)
