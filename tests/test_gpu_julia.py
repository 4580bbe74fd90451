"""The Julia render (include/cudabrot_amd.h, "Julia render") on the GPU.  Every case three ways -- the product kernel
(cb_debug_last_draw_kernel 12), the lock-step kernel (13), the CPU restatement (tests/plot_reference.c) -- bit for bit on
histogram, generator states and every counter but skipped_steps:

  1. the parameters c that matter (a connected set, superattracting and parabolic interiors, dust, the ends of the
     range), each step, another plane on a cropped canvas;
  2. the edges of the iteration control, of the grid and of the canvas;
  3. everything the ABI refuses;
  4. the renderer and the binary.
"""

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

PRODUCT, LOCKSTEP = 12, 13


def three_ways(cb, ref, oracle, c, degree=2, ship=False, max_iter=500, min_iter=20, w=256, h=256, box=SQUARE, threads=4096,
               launches=(50,), projection=plot.IDENTITY):
    """Product == lock-step == restatement, without an interior map -> (restatement's counters, product's counters,
    lock-step's counters)."""
    r = plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), 0, w, h, box, max_iter, min_iter, threads, launches,
                                c=c, degree=degree, ship=ship, projection=projection)
    return r.wc, r.product, r.lockstep


# ---- 1. the parameters -------------------------------------------------------------------------------------------------


def test_connected_set(cb, ref, oracle):
    wc, _, _ = three_ways(cb, ref, oracle, (-0.8, 0.156), max_iter=500, min_iter=20, launches=[100])
    assert wc["recorded"] > 10000  # about 10 % of the samples have k >= 20


def test_hologram_on_a_cropped_canvas_takes_its_constant_from_the_fixed_c(cb, ref, oracle):
    wc, _, _ = three_ways(cb, ref, oracle, (-0.8, 0.156), max_iter=500, min_iter=20, w=300, h=200,
                          box=(-1.3, 0.9, -0.7, 0.55), launches=[100], projection=plot.HOLOGRAM)
    assert wc["recorded"] > 10000 and 0 < wc["increments"] < wc["replay_steps"]  # points on the canvas and off it


def test_c_zero_reaches_the_exact_fixed_point(cb, ref, oracle):
    wc, product, lockstep = three_ways(cb, ref, oracle, (0.0, 0.0), max_iter=2000, min_iter=0)
    assert wc["never_escaped"] > 20000  # the unit disc: about 19.6 % of the square
    assert product["skipped_steps"] > 0
    assert product["iterate_steps"] - product["skipped_steps"] < lockstep["iterate_steps"] == wc["iterate_steps"]


def test_superattracting_two_cycle(cb, ref, oracle):
    wc, product, _ = three_ways(cb, ref, oracle, (-1.0, 0.0), max_iter=2000, min_iter=1)
    assert wc["never_escaped"] > 0
    assert product["skipped_steps"] > 0


def test_parabolic_interior(cb, ref, oracle):
    wc, _, _ = three_ways(cb, ref, oracle, (-0.75, 0.0), max_iter=1000, min_iter=0)
    assert wc["never_escaped"] > 0  # (no exact cycle is expected: nothing is asserted about skipped_steps)


def test_dust(cb, ref, oracle):
    wc, _, _ = three_ways(cb, ref, oracle, (0.5, 0.5), max_iter=300, min_iter=0)
    assert wc["never_escaped"] * 100 < wc["samples"] and wc["recorded"] > 0


@pytest.mark.parametrize("c", [(-2.0, 0.0), (2.0, 2.0)], ids=["minus2", "corner"])
def test_ends_of_the_c_range(cb, ref, oracle, c):
    wc, _, _ = three_ways(cb, ref, oracle, c, max_iter=300, min_iter=0, w=64, h=64)
    assert wc["recorded"] > 0 and wc["increments"] > 0


def test_ship_step(cb, ref, oracle):
    wc, _, _ = three_ways(cb, ref, oracle, (-0.8, 0.156), ship=True, max_iter=500, min_iter=0)
    assert wc["recorded"] > 0 and wc["increments"] > 0


@pytest.mark.parametrize("degree,c", [(3, (0.0, 0.0)), (8, (0.4, 0.2))], ids=["d3", "d8"])
def test_multibrot_steps(cb, ref, oracle, degree, c):
    wc, _, _ = three_ways(cb, ref, oracle, c, degree=degree, max_iter=500, min_iter=0)
    assert wc["never_escaped"] > 0 and wc["recorded"] > 0 and wc["increments"] > 0


@pytest.mark.parametrize("degree", [4, 5, 6, 7])
def test_the_other_degrees_are_their_own_instances(cb, ref, oracle, degree):
    wc, _, _ = three_ways(cb, ref, oracle, (0.3, -0.2), degree=degree, max_iter=100, min_iter=0, w=64, h=64, threads=1024,
                          launches=[20])
    assert wc["recorded"] > 0


# ---- 2. edges -----------------------------------------------------------------------------------------------------------

EDGES = {
    "max0": dict(max_iter=0, min_iter=0),
    "max1": dict(max_iter=1, min_iter=0),
    "min_is_max_minus_1": dict(max_iter=50, min_iter=49),
    "window_of_two": dict(max_iter=3, min_iter=1),
    "ragged_4000": dict(threads=4000),
    "two_launches": dict(launches=[50, 70]),
    "333x77": dict(w=333, h=77, box=(-1.6, 0.9, -0.7, 0.55)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(cb, ref, oracle, name):
    shape = dict(max_iter=200, min_iter=5, w=128, h=128, threads=2048, launches=[50])
    shape.update(EDGES[name])
    wc, _, _ = three_ways(cb, ref, oracle, (-0.8, 0.156), **shape)
    if name == "max0":
        assert wc["never_escaped"] == wc["samples"] and wc["iterate_steps"] == 0 and wc["increments"] == 0
    elif name == "max1":  # only k == 0 is accepted: one replayed point, z_1
        assert wc["recorded"] > 0 and wc["replay_steps"] == wc["recorded"] and wc["never_escaped"] > 0
    elif name == "min_is_max_minus_1":  # only k == 49
        assert wc["replay_steps"] == 50 * wc["recorded"]
    elif name == "window_of_two":  # k == 1 or k == 2
        assert wc["recorded"] > 0 and 2 * wc["recorded"] <= wc["replay_steps"] <= 3 * wc["recorded"]
    else:
        assert wc["recorded"] > 0 and wc["too_fast"] > 0 and wc["increments"] > 0


# ---- 3. what the ABI refuses --------------------------------------------------------------------------------------------


def test_julia_launches_refuse_what_they_do_not_define(cb):
    import torch

    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, threads, no_counters=True)
    buf, states = bufs.out, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_matrix = (C.c_double * 8)(*([float("nan")] + list(cb.IDENTITY_PROJECTION[1:])))
    c_good = (C.c_double * 2)(-0.8, 0.156)
    d, b, i, s = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr()

    def draw(c, variant, p=good):
        return cb.lib.cb_draw_buddhabrot_julia(d, b, i, p, c, s, threads, 5, None, variant, None)

    nan, inf = float("nan"), float("inf")
    for c in ((2.5, 0.0), (0.0, 2.5), (-2.0000001, 0.0), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert draw((C.c_double * 2)(*c), base) == INVALID, c
    assert draw(None, 0) == INVALID and draw(c_good, 0, None) == INVALID and draw(c_good, 0, bad_matrix) == INVALID
    power3 = cb.CB_KERNEL_POWER(3)
    bad_variants = [cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_TIMED,
                    cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_DRAIN, power3 | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                    power3 | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP, power3 | cb.CB_KERNEL_FLAG_ANTI,
                    2 << 12, 9 << 12, 15 << 12]
    for variant in bad_variants:
        assert draw(c_good, variant) == INVALID, variant
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success
    assert cb.lib.cb_draw_buddhabrot_julia(d, b, i, good, c_good, s, threads, 0, None, 0, None) == 0
    assert cb.lib.cb_draw_buddhabrot_julia(d, b, i, good, c_good, s, 0, 5, None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)


def test_renderer_refuses_julia_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    c_good = (C.c_double * 2)(-0.8, 0.156)
    out = (C.c_double * 2)(7.0, 7.0)
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID  # a channel renderer
        assert r.julia() is None
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID  # a focused renderer
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID  # a projected renderer
        assert r.julia() is None
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        r.render_passes(1)
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID  # after the first pass
    with cb.Renderer(dims, it, device=0, n_threads=1024) as r:
        fresh = r.read_rng_states().copy()
        assert cb.lib.cb_renderer_julia(r._h, out) == 0 and list(out) == [7.0, 7.0]
        for c in ((2.5, 0.0), (float("nan"), 0.0), (0.0, float("-inf"))):
            assert cb.lib.cb_renderer_set_julia(r._h, good, (C.c_double * 2)(*c)) == INVALID
        assert cb.lib.cb_renderer_set_julia(r._h, good, None) == INVALID
        bad = list(cb.IDENTITY_PROJECTION)
        bad[5] = float("inf")
        assert cb.lib.cb_renderer_set_julia(r._h, (C.c_double * 8)(*bad), c_good) == INVALID
        assert r.julia() is None and r.projection() is None
        r.set_julia((-0.8, 0.156))  # NULL matrix: the identity
        assert r.julia() == (-0.8, 0.156)
        assert np.array_equal(r.projection().reshape(-1), np.array(cb.IDENTITY_PROJECTION))
        assert cb.lib.cb_renderer_set_julia(r._h, good, c_good) == INVALID  # once
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == INVALID
        assert cb.lib.cb_renderer_set_projection(r._h, good) == INVALID
        for variant in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FULL_ITERATE, 9 << 12,
                        cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        assert int(r.read_histogram().sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)


# ---- 4. the renderer and the binary ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("degree", [2, 3])
def test_julia_renderer_over_several_calls(cb, ref, oracle, base, degree):
    w, h, box, m, mn, threads, c = 300, 200, (-2.0, 1.0, -2.0, 1.0), 400, 10, 4096, (-0.8, 0.156)
    p = plot.HOLOGRAM
    variant = variant_of(cb, base, degree, False)
    st = oracle.init_states(1337, 0, threads)
    want, wc = plot.draw(ref, w, h, m, mn, threads, [50] * 4, c=c, degree=degree, projection=p, box=box,
                         omp_threads=omp_threads(), states=st)
    dims = cb.FractalDimensions.make(w, h, *box)
    with cb.Renderer(dims, cb.IterationControl(m, mn), device=0, n_threads=threads) as r:
        r.set_julia(c, p)
        r.prepare(variant)  # must not fail
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(3, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        assert cb.lib.cb_renderer_interior_map_level(r._h) == 0
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        states = r.read_rng_states().view(np.uint32)
    assert wc["recorded"] > 100 and wc["increments"] > 100  # not empty
    assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == wc, (cnt, wc)
    assert np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))


def test_cli_julia_buffer_equals_the_restatement_and_resumes(exe, ref, tmp_path):
    common = ["--julia", "-0.8,0.156", "-w", "256", "-h", "256", "-m", "500", "-c", "20", "-o", os.devnull]
    one_buf, one_side = str(tmp_path / "one.bin"), str(tmp_path / "one.rng")
    r = run(exe, "--passes", "2", "-s", one_buf, "--rng-state", one_side, "--stats", *common)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert [float.fromhex(v) for v in json.loads(lines[1])["julia"]] == [-0.8, 0.156]
    want, wc = plot.draw(ref, 256, 256, 500, 20, 512 * 512, [100], c=(-0.8, 0.156), omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    assert wc["recorded"] > 100000
    assert np.array_equal(read_state_file(one_buf, 256, 256), want)
    # one pass, the two files written, then one more pass on them: the same run
    buf, side = str(tmp_path / "two.bin"), str(tmp_path / "two.rng")
    assert run(exe, "--passes", "1", "-s", buf, "--rng-state", side, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 1 passes." in r2.stdout, r2.stdout
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        assert a.read() == b.read()
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()


def test_cli_julia_with_power_on_another_plane(exe, ref, tmp_path):
    buf = str(tmp_path / "p.bin")
    r = run(exe, "--julia", "-0.8,0.156", "--power", "3", "--plane", "zr,cr", "--passes", "1", "-w", "256", "-h", "256",
            "-m", "500", "-c", "20", "-s", buf, "--stats", "-o", os.devnull)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert json.loads(lines[1]) == {"power": 3} and "julia" in json.loads(lines[2])
    want, wc = plot.draw(ref, 256, 256, 500, 20, 512 * 512, [50], c=(-0.8, 0.156), degree=3, projection=plot.ZR_CR,
                         omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    assert np.array_equal(read_state_file(buf, 256, 256), want)
