"""The bounded render (include/cudabrot_amd.h, "Bounded render") on the GPU:

  1. three ways -- the product kernel (cb_debug_last_draw_kernel 26), the lock-step kernel (27), the CPU restatement
     (tests/bounded_reference.c) -- bit for bit on histogram, generator states and every counter but skipped_steps, and the
     product's skipped_steps is the compressed restatement's, to the step;
  2. the inputs reach the paths: escapers, exact cycles, bounded orbits without one, cycles with both weights, points off
     the canvas;
  3. the identity with a sampled c is the anti-Buddhabrot (kernels 4 and 5), and consecutive launches add up;
  4. everything the ABI refuses;
  5. the renderer: its new column, what a bounded renderer refuses, and the renderer against the entry point;
  6. the binary.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from bounded_harness import (KEYS, LAUNCHES, LOCKSTEP, MAX, MIN, PRODUCT, THREADS, H, W, bounded_launches, bref,  # noqa: F401
                             shape_of, three_ways)
from conftest import read_state_file
from plot_harness import INVALID, SAME, SQUARE, exe  # noqa: F401
from plot_harness import gpu_run as run
from test_gpu_renderer_kinds import getters, library_planes, make

pytestmark = pytest.mark.gpu

CROP = (-1.5, 0.7, -0.9, 1.1)
# the z_re, z_im plane turned by three angles: two unit rows with four irrational entries each
ROTATED = plot.rotate(plot.rotate(plot.rotate(plot.IDENTITY, "zr", "zi", 25.0), "zr", "cr", 40.0), "zi", "ci", 55.0)
RABBIT = (-0.123, 0.745)
CASES = {
    "reference_zr_cr": dict(projection=plot.ZR_CR, box=CROP),
    "ship_identity": dict(ship=True, box=CROP),
    "cubic_rotated": dict(degree=3, projection=ROTATED, box=CROP),
    "tricorn": dict(formula="tricorn", box=CROP),
    "julia_basilica_identity": dict(c=(-1.0, 0.0)),
    "julia_basilica_zr_cr": dict(c=(-1.0, 0.0), projection=plot.ZR_CR),
    "julia_rabbit_identity": dict(c=RABBIT, box=CROP),
    "julia_rabbit_zr_cr": dict(c=RABBIT, projection=plot.ZR_CR),
    "julia_cubic": dict(c=(-0.1, 0.6), degree=3, box=CROP),
    # the rabbit's slowest orbits are not yet on an exact cycle at k = 60, and -m 130 ends before the next comparison
    "julia_rabbit_max_130": dict(c=RABBIT, max_iter=130),
}
SAMPLED = [name for name, kw in CASES.items() if "c" not in kw]


# ---- 1, 2. three ways, on inputs that reach the paths --------------------------------------------------------------------


@pytest.fixture(scope="module")
def cases(cb, bref, oracle):  # noqa: F811
    """Every case three ways, once for the module."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = three_ways(cb, bref, oracle, **CASES[name])
        return done[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_three_ways(cases, name):
    want, wc, extra, product = cases(name)
    assert wc["recorded"] > 0 and wc["increments"] > 0 and want.any()
    assert extra["escaped"] > 0 and extra["cycles"] > 0 and product["skipped_steps"] > 0


@pytest.mark.parametrize("name", SAMPLED)
def test_a_sampled_c_reaches_every_path(cases, name):
    _, _, extra, _ = cases(name)
    for key in ("escaped", "cycles", "no_cycle", "both_weights", "off_canvas", "in_canvas"):
        assert extra[key] > 0, (key, extra)


def test_a_fixed_c_has_cycle_less_bounded_orbits_at_a_small_max_only(cases):
    assert cases("julia_rabbit_identity")[2]["no_cycle"] == 0
    extra = cases("julia_rabbit_max_130")[2]
    assert extra["no_cycle"] > 0 and extra["cycles"] > 0 and extra["both_weights"] > 0


def test_a_fixed_c_on_zr_cr_is_one_row(cases):
    want = cases("julia_basilica_zr_cr")[0]
    rows = np.flatnonzero(want.sum(axis=1))
    assert len(rows) == 1 and abs(int(rows[0]) - H // 4) <= 1  # v = c_re = -1 for every point


# ---- 3. identities -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ship", [False, True], ids=["plain", "ship"])
def test_the_identity_with_a_sampled_c_is_the_anti_buddhabrot(cb, ship):
    flags = cb.CB_KERNEL_FLAG_ANTI | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        hist, cnt, kernel, states = bounded_launches(cb, base, ship=ship, box=CROP)
        assert kernel == PRODUCT + base and cnt["status"] == 0 and cnt["recorded"] > 0
        for anti_base, anti_kernel in ((cb.CB_KERNEL_DEFAULT, 4), (cb.CB_KERNEL_SIMPLE, 5)):
            ah, ac, launched, ast = plot_harness.gpu_launches(cb, W, H, CROP, MAX, MIN, THREADS, LAUNCHES, anti_base | flags,
                                                              projection=None)
            assert launched == anti_kernel and ac["status"] == 0
            assert np.array_equal(hist, ah) and np.array_equal(states, ast)
            assert {k: cnt[k] for k in SAME} == {k: ac[k] for k in SAME}
            if base == anti_base:  # the same schedule: the same steps saved
                assert cnt["skipped_steps"] == ac["skipped_steps"]


def test_consecutive_launches_equal_one_launch_of_the_sum(cb):
    for kw in (dict(projection=ROTATED, box=CROP), dict(c=RABBIT, projection=plot.HOLOGRAM)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            a = bounded_launches(cb, base, launches=(3, 50, 1), **kw)
            b = bounded_launches(cb, base, launches=(54,), **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
            assert {k: a[1][k] for k in KEYS} == {k: b[1][k] for k in KEYS}
            assert a[1]["recorded"] > 0


def test_min_escape_iterations_is_not_read(cb):
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        a = bounded_launches(cb, base, min_iter=0, launches=(20,))
        b = bounded_launches(cb, base, min_iter=MAX + 100, launches=(20,))
        assert np.array_equal(a[0], b[0]) and {k: a[1][k] for k in KEYS} == {k: b[1][k] for k in KEYS}
        assert a[1]["increments"] > 0


# ---- 4. what the ABI refuses ---------------------------------------------------------------------------------------------


def test_bounded_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads)
    buf, states, counters = bufs.out, bufs.states, bufs.counters
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(-1.0, 0.0)
    d, b, i, s = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr()

    def draw(variant=0, c=None, m=good, samples=5):
        return cb.lib.cb_draw_buddhabrot_bounded(d, b, i, m, c, s, threads, samples, counters.data_ptr(), variant, None)

    nan, inf = float("nan"), float("inf")
    power3, tricorn, ship = cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA(1), cb.CB_KERNEL_FLAG_BURNING_SHIP
    flags = [cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FLAG_ANTI | ship, power3 | ship,
             cb.CB_KERNEL_POWER(8) | ship, tricorn | ship, tricorn | power3, cb.CB_KERNEL_FORMULA(5) | cb.CB_KERNEL_POWER(8),
             tricorn | cb.CB_KERNEL_FLAG_ANTI, power3 | cb.CB_KERNEL_FLAG_DRAIN, 2 << 12, 9 << 12, 6 << 16]
    for flag in flags:
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            for c in (None, c_good):
                assert draw(base | flag, c=c) == INVALID, (base, flag)
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED | ship, cb.CB_KERNEL_FULL_ITERATE | power3):
        for c in (None, c_good):
            assert draw(variant, c=c) == INVALID, variant
    for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, nan), (0.0, inf), (-inf, 0.0)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw(base, c=(C.c_double * 2)(*c)) == INVALID, c
    for j in range(8):
        for bad in (nan, inf):
            m = list(cb.IDENTITY_PROJECTION)
            m[j] = bad
            assert draw(m=(C.c_double * 8)(*m)) == INVALID
    assert draw(m=None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_bounded(None, b, i, good, None, s, threads, 5, counters.data_ptr(), 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_bounded(d, None, i, good, None, s, threads, 5, counters.data_ptr(), 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_bounded(d, b, None, good, None, s, threads, 5, counters.data_ptr(), 0, None) == INVALID
    assert cb.lib.cb_draw_buddhabrot_bounded(d, b, i, good, None, None, threads, 5, counters.data_ptr(), 0, None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success
    assert draw(samples=0) == 0
    assert cb.lib.cb_draw_buddhabrot_bounded(d, b, i, good, None, s, 0, 5, counters.data_ptr(), 0, None) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)
    # every variant cb_draw_buddhabrot_julia accepts, with either source; the bounds of c are allowed
    accepted = [0, ship, tricorn, cb.CB_KERNEL_FORMULA(5)] + [cb.CB_KERNEL_POWER(deg) for deg in range(3, 9)]
    n = 0
    for flag in accepted:
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            for c in (None, c_good, (C.c_double * 2)(2.0, -2.0)):
                assert draw(base | flag, c=c) == 0, (base, flag)
                n += 1
    torch.cuda.synchronize()
    cnt = bufs.read_counters()
    assert cnt["samples"] == n * 5 * threads and cnt["status"] == 0 and cnt["rejected"] == 0
    assert int(buf.sum()) == cnt["increments"] > 0


# ---- 5. the renderer -----------------------------------------------------------------------------------------------------

# cb_renderer_set_bounded on the starting renderers of tests/test_gpu_renderer_kinds.py: 1 accepted, 0 refused -- literal data
BOUNDED_COLUMN = {
    "plain": 1,
    "channels": 0,
    "focused": 0,
    "projected": 1,
    "julia": 1,
    "plain + palette": 0,
    "projected + palette": 0,
    "julia + palette": 0,
    "projected + depth": 0,
    "julia + depth palette": 0,
    "projected + frames": 0,
    "julia + phoenix": 0,
    "plain after a pass": 0,
    "projected after a pass": 0,
}


@pytest.mark.parametrize("name", list(BOUNDED_COLUMN))
def test_set_bounded_on_every_starting_renderer(cb, name):
    accepted = BOUNDED_COLUMN[name]
    with make(cb, name, name == "focused") as r:
        h, w = r.dims.h, r.dims.w
        before, hist = getters(r), r.read_histogram()
        assert not r.bounded()
        code = cb.lib.cb_renderer_set_bounded(r._h)
        if not accepted:
            assert code == INVALID and not r.bounded()
            assert getters(r) == before
            after = r.read_histogram()
            assert after.shape == hist.shape and np.array_equal(after, hist)
            assert library_planes(cb, r) == (hist.shape[0] if hist.ndim == 3 else 1)
            return
        assert code == 0 and r.bounded()
        # the source of c stays; a plain renderer gains the identity, as with a palette
        now = getters(r)
        assert now[1:] == before[1:] and np.ravel(now[0]).tolist() == list(cb.IDENTITY_PROJECTION)
        assert r.read_histogram().shape == (h, w) and library_planes(cb, r) == 1
        assert cb.lib.cb_renderer_set_bounded(r._h) == INVALID  # once
        r.render_passes(1)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT and cb.lib.cb_renderer_interior_map_level(r._h) == 0
        cnt = r.read_counters().as_dict()
        assert int(r.read_histogram().sum()) == cnt["increments"] and cnt["status"] == 0 and cnt["rejected"] == 0
        assert cnt["increments"] > 0 and cnt["recorded"] > 0


def test_a_bounded_renderer_refuses_all_nine_setters(cb):
    dims, it = cb.FractalDimensions.make(16, 16), cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(-1.0, 0.0)
    p_good = (C.c_double * 2)(-0.5, 0.0)
    depth = cb.Depth.make("cr", -2.0, 0.5, 4)
    table = np.ascontiguousarray(plot.demo_table(100), dtype=np.uint32)
    slice_table = np.ascontiguousarray(plot.demo_table(4), dtype=np.uint32)
    frames = np.ascontiguousarray([cb.IDENTITY_PROJECTION] * 2, dtype=np.float64)
    setters = {
        "focus": lambda r: cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0),
        "projection": lambda r: cb.lib.cb_renderer_set_projection(r._h, good),
        "julia": lambda r: cb.lib.cb_renderer_set_julia(r._h, good, c_good),
        "palette": lambda r: cb.lib.cb_renderer_set_palette(r._h, table.ctypes.data, table.size),
        "depth": lambda r: cb.lib.cb_renderer_set_depth(r._h, C.byref(depth)),
        "depth_palette": lambda r: cb.lib.cb_renderer_set_depth_palette(r._h, C.byref(depth), slice_table.ctypes.data, 4),
        "frames": lambda r: cb.lib.cb_renderer_set_frames(r._h, frames.ctypes.data, 2),
        "phoenix": lambda r: cb.lib.cb_renderer_set_phoenix(r._h, p_good),
        "bounded": lambda r: cb.lib.cb_renderer_set_bounded(r._h),
    }
    for start in ("plain", "projected", "julia"):
        with cb.Renderer(dims, it, device=0, n_threads=256) as r:
            if start == "projected":
                r.set_projection(plot.ZR_CR)
            elif start == "julia":
                r.set_julia((-1.0, 0.0), plot.ZR_CR)
            r.set_bounded()
            before = getters(r)
            fresh = r.read_rng_states().copy()
            for name, setter in setters.items():
                assert setter(r) == INVALID, (start, name)
                assert getters(r) == before and r.bounded(), (start, name)
            # render_passes and prepare take what the entry point takes
            for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED,
                            cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
                assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID, variant
            hist = r.read_histogram()
            assert hist.shape == (16, 16) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
            assert np.array_equal(r.read_rng_states(), fresh)
            r.render_passes(1, cb.CB_KERNEL_FORMULA(1))  # and it renders, with a step of the plotted path
            assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT
            assert int(r.read_histogram().sum()) == r.read_counters().as_dict()["increments"] > 0


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", ["reference_zr_cr", "cubic_rotated", "julia_rabbit_identity", "plain"])
def test_renderer_against_the_entry_point_on_identical_passes(cb, base, name):
    kw = shape_of(dict(box=CROP) if name == "plain" else CASES[name])
    kw.update(launches=(50, 100))  # one pass, then two fused: the same samples per generator
    want, wc, kernel, states = bounded_launches(cb, base, **kw)
    variant = plot_harness.variant_of(cb, base, kw["degree"], kw["ship"], plot.code_of(kw["formula"]))
    dims = cb.FractalDimensions.make(kw["w"], kw["h"], *kw["box"])
    with cb.Renderer(dims, cb.IterationControl(MAX, MIN), device=0, n_threads=THREADS) as r:
        if name == "plain":
            pass  # set_bounded alone brings the identity
        elif kw["c"] is None:
            r.set_projection(kw["projection"])
        else:
            r.set_julia(kw["c"], kw["projection"])
        assert not r.bounded()
        r.set_bounded()
        assert r.bounded() and r.julia() == (None if kw["c"] is None else tuple(kw["c"]))
        assert np.ravel(r.projection()).tolist() == plot.matrix(kw["projection"]).tolist()
        r.prepare(variant)  # must not fail
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(2, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == kernel == PRODUCT + base
        assert cb.lib.cb_renderer_interior_map_level(r._h) == 0
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        after = r.read_rng_states().view(np.uint32)
        assert hist.shape == (kw["h"], kw["w"])
        assert cnt["status"] == 0 and {k: cnt[k] for k in KEYS} == {k: wc[k] for k in KEYS}
        assert wc["recorded"] > 0 and np.array_equal(hist, want) and np.array_equal(after, states)
        # the image is the one plane's: the reference's tone map of the histogram
        for gamma in (1.0, 2.2):
            gray, mx, scale = r.grayscale_image(gamma)
            want_gray, want_max, want_scale = cb.set_grayscale_pixels(hist, gamma)
            assert mx == want_max == int(hist.max()) > 0 and scale == want_scale
            assert np.array_equal(gray.astype(np.uint16), want_gray)
        # the buffer and the generators go out and come back as for a projected renderer
        r.write_histogram(hist)
        r.write_rng_states(r.read_rng_states())
        assert np.array_equal(r.read_histogram(), hist)


# ---- 6. the binary -------------------------------------------------------------------------------------------------------

CLI_W, CLI_H, CLI_MAX, CLI_MIN = 64, 48, 130, 10


def api_render(cb, passes, variant=0, c=None, projection=None):
    """What the binary's run is: a renderer of its default threads and seed -> (hist, counters)."""
    dims = cb.FractalDimensions.make(CLI_W, CLI_H)
    with cb.Renderer(dims, cb.IterationControl(CLI_MAX, CLI_MIN), device=0) as r:
        if c is not None:
            r.set_julia(c, projection)
        elif projection is not None:
            r.set_projection(projection)
        r.set_bounded()
        r.render_passes(passes, variant)
        return r.read_histogram(), r.read_counters().as_dict()


CLI_COMMON = ["--bounded", "-w", str(CLI_W), "-h", str(CLI_H), "-m", str(CLI_MAX), "-c", str(CLI_MIN), "-o", os.devnull]


@pytest.fixture(scope="module")
def three_passes(cb):
    """Three passes of the binary's run through the API, once for the module -> (hist, counters)."""
    want, wc = api_render(cb, 3)
    assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT and wc["recorded"] > 0 and wc["skipped_steps"] > 0
    return want, wc


def test_cli_bounded_equals_the_api_and_resumes(exe, tmp_path, three_passes):  # noqa: F811
    common, (want, wc) = CLI_COMMON, three_passes
    one_buf, one_side = str(tmp_path / "one.bin"), str(tmp_path / "one.rng")
    r = run(exe, "--passes", "3", "-s", one_buf, "--rng-state", one_side, "--stats", *common)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"bounded": True}
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in KEYS} == {k: wc[k] for k in KEYS}
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


def test_cli_bounded_ignores_c_round_trips_the_raw_format_and_selects_its_kernels(cb, exe, tmp_path, three_passes):  # noqa: F811
    common, (want, wc) = CLI_COMMON, three_passes
    # -c is not read, as under --anti
    other = str(tmp_path / "c.bin")
    assert run(exe, "--passes", "3", "-s", other, *[a if a != str(CLI_MIN) else "120" for a in common]).returncode == 0
    assert np.array_equal(read_state_file(other, CLI_H, CLI_W), want)
    # the raw format is the one plane's, and it is read back: two passes, then one more on the files
    raw, side = str(tmp_path / "raw.bin"), str(tmp_path / "raw.rng")
    assert run(exe, "--passes", "2", "-s", raw, "--state-format", "raw", "--rng-state", side, *common).returncode == 0
    r4 = run(exe, "--passes", "1", "-s", raw, "--state-format", "raw", "--rng-state", side, *common)
    assert r4.returncode == 0, r4.stdout + r4.stderr
    assert np.array_equal(np.fromfile(raw, dtype=np.uint32).reshape(CLI_H, CLI_W), want)
    # --kernel simple is the lock-step kernel (27): the same buffer and counters, and nothing skipped; the default is the
    # product kernel (26), whose compression shows in skipped_steps
    simple = str(tmp_path / "simple.bin")
    r3 = run(exe, "--kernel", "simple", "--passes", "3", "-s", simple, "--stats", *common)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    stats3 = json.loads(r3.stderr.strip().split("\n")[-1])
    assert {k: stats3[k] for k in SAME} == {k: wc[k] for k in SAME} and stats3["skipped_steps"] == 0 < wc["skipped_steps"]
    assert np.array_equal(read_state_file(simple, CLI_H, CLI_W), want)
    lock, lc = api_render(cb, 3, cb.CB_KERNEL_SIMPLE)
    assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP and lc["skipped_steps"] == 0 and np.array_equal(lock, want)


@pytest.mark.parametrize("flags,variant,c,projection", [
    (["--plane", "zr,cr"], 0, None, plot.ZR_CR),
    (["--julia", "-1,0", "--plane", "zr,zi", "--rotate", "zi,cr:90"], 0, (-1.0, 0.0), ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))),
    (["--power", "3", "--plane", "zi,ci"], "power3", None, ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))),
    (["--formula", "tricorn"], "tricorn", None, None),
    (["--burning-ship"], "ship", None, None),
], ids=["zr_cr", "julia_rotated", "cubic_zi_ci", "tricorn", "ship"])
def test_cli_bounded_with_the_flags_it_combines_with(cb, exe, tmp_path, flags, variant, c, projection):  # noqa: F811
    variant = {0: 0, "power3": cb.CB_KERNEL_POWER(3), "tricorn": cb.CB_KERNEL_FORMULA(1),
               "ship": cb.CB_KERNEL_FLAG_BURNING_SHIP}[variant]
    buf = str(tmp_path / "b.bin")
    r = run(exe, "--bounded", *flags, "--passes", "1", "-w", str(CLI_W), "-h", str(CLI_H), "-m", str(CLI_MAX), "-c",
            str(CLI_MIN), "-s", buf, "--stats", "-o", os.devnull)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '{"bounded": true}' in r.stderr.split("\n")
    want, wc = api_render(cb, 1, variant, c=c, projection=projection)
    stats = json.loads(r.stderr.strip().split("\n")[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in KEYS} == {k: wc[k] for k in KEYS}
    assert wc["recorded"] > 0 and wc["increments"] > 0 and np.array_equal(read_state_file(buf, CLI_H, CLI_W), want)
