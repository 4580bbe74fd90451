"""The projected render (include/cudabrot_amd.h, "Projected render") on the GPU, bit for bit on histogram, generator
states and counters (all but skipped_steps and the clocks):

  1. the identity matrix against the normal path (cb_draw_buddhabrot: its lock-step kernel and its default product path);
  2. general matrices: product kernel == lock-step kernel == the CPU restatement (tests/plot_reference.c);
  3. the early-outs (interior map, exact periodicity) change nothing but the executed work;
  4. the renderer (set_projection, several calls, resume) and the binary against the restatement.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import SAME, SQUARE, exe, omp_threads, planar_states, ref  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 8, 9


def same(a, b):
    return {k: a[k] for k in SAME} == {k: b[k] for k in SAME}


def gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, base, ship=False, projection=None):
    """plot_harness.gpu_launches, projected, or -- projection=None -- through cb_draw_buddhabrot."""
    return plot_harness.gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches,
                                     plot_harness.variant_of(cb, base, ship=ship), projection=projection)


# ---- 1. the identity matrix is a normal render ---------------------------------------------------------------------------

# (w, h, box, ship, threads, max_iter, min_iter, launches)
IDENTITY_CASES = {
    "dyadic": (256, 256, SQUARE, False, 4096, 500, 20, [100]),
    "cropped": (300, 200, (-1.9, -0.7, -0.45, 0.35), False, 4096, 500, 20, [100]),  # deltas 0.004: not powers of two
    "333x77": (333, 77, SQUARE, False, 4096, 300, 10, [100]),
    "ship": (256, 256, SQUARE, True, 4096, 500, 20, [100]),
    "ragged": (256, 256, SQUARE, False, 4000, 1000, 20, [100]),
    "min_iter_0": (256, 256, SQUARE, False, 2048, 100, 0, [100]),
    "min_is_max_minus_1": (256, 256, SQUARE, False, 2048, 50, 49, [200]),
    "window_of_two": (256, 256, SQUARE, False, 2048, 3, 1, [100]),
    "max_iter_0": (128, 128, SQUARE, False, 2048, 0, 0, [50]),
    "max_iter_1": (128, 128, SQUARE, False, 2048, 1, 0, [100]),
    "max_iter_1_ship": (128, 128, SQUARE, True, 2048, 1, 0, [100]),
    "two_launches": (256, 256, SQUARE, False, 4096, 2000, 200, [50, 70]),
    "two_launches_ship": (200, 300, (-2.2, 1.4, -2.0, 0.9), True, 3000, 700, 30, [30, 50]),
}


@pytest.mark.parametrize("case", list(IDENTITY_CASES))
def test_identity_matrix_equals_the_normal_path(cb, case):
    w, h, box, ship, threads, max_iter, min_iter, launches = IDENTITY_CASES[case]
    args = (cb, w, h, box, max_iter, min_iter, threads, launches)
    normal = {}
    for name, base in (("lockstep", cb.CB_KERNEL_SIMPLE), ("product", cb.CB_KERNEL_DEFAULT)):
        normal[name] = gpu_launches(*args, base, ship)
    assert normal["lockstep"][2] == 3 and normal["product"][2] in (1, 2)
    for base, kernel in ((cb.CB_KERNEL_DEFAULT, PRODUCT), (cb.CB_KERNEL_SIMPLE, LOCKSTEP)):
        hist, cnt, launched, states = gpu_launches(*args, base, ship, projection=cb.IDENTITY_PROJECTION)
        assert launched == kernel
        assert cnt["status"] == 0
        for name, (want, wc, _, want_states) in normal.items():
            assert wc["status"] == 0
            assert same(cnt, wc), (name, cnt, wc)
            assert np.array_equal(hist, want), name
            assert np.array_equal(states, want_states), name
        assert int(hist.sum()) == cnt["increments"]
        if kernel == LOCKSTEP:
            assert cnt["skipped_steps"] == 0
    if max_iter >= 100:
        assert normal["lockstep"][1]["increments"] > 0 and normal["lockstep"][1]["recorded"] > 0


def test_projected_launches_refuse_what_they_do_not_define(cb):
    import torch

    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = plot_harness.Launches(cb, dims, 64, no_counters=True)
    buf, states = bufs.out, bufs.states
    torch.cuda.synchronize()
    draw = cb.lib.cb_draw_buddhabrot_projected
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN,
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI):
        assert draw(C.byref(dims), buf.data_ptr(), C.byref(it), good, states.data_ptr(), 64, 1, None, variant, None) == 1
    for index in range(8):
        for bad in (float("nan"), float("inf"), float("-inf")):
            p = list(cb.IDENTITY_PROJECTION)
            p[index] = bad
            assert draw(C.byref(dims), buf.data_ptr(), C.byref(it), (C.c_double * 8)(*p), states.data_ptr(), 64, 1, None,
                        0, None) == 1
    assert draw(C.byref(dims), buf.data_ptr(), C.byref(it), None, states.data_ptr(), 64, 1, None, 0, None) == 1
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ---- 2. general matrices against the restatement ---------------------------------------------------------------------------

MATRICES = {"c_plane": plot.C_PLANE, "zr_cr": plot.ZR_CR, "hologram": plot.HOLOGRAM}


@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "ship"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_general_matrix_equals_the_restatement(cb, ref, oracle, name, ship):
    w, h, box, max_iter, min_iter, threads, launches = 320, 240, (-2.0, 1.5, -1.75, 1.75), 600, 15, 4000, [50, 70]
    # the interior map is the Mandelbrot set's: the product kernel consults it (level 8 or above) unless the step is the ship's
    want, wc, _, _, _ = plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), 0 if ship else 8, w, h, box, max_iter,
                                                min_iter, threads, launches, ship=ship, projection=MATRICES[name])
    assert wc["increments"] > 1000
    if name == "c_plane":  # every accepted sample's k + 1 points on the one pixel of c
        assert int(want.sum()) == wc["increments"] <= wc["replay_steps"]


# ---- 3. the early-outs change nothing but the work ---------------------------------------------------------------------------


def test_early_outs_change_only_the_executed_work(cb, monkeypatch):
    w, h, box, max_iter, min_iter, threads, launches = 256, 256, SQUARE, 20000, 20, 4096, [50]
    p = plot.HOLOGRAM
    args = (cb, w, h, box, max_iter, min_iter, threads, launches)
    with_map = gpu_launches(*args, cb.CB_KERNEL_DEFAULT, projection=p)
    assert cb.lib.cb_debug_interior_map_level() >= 8
    monkeypatch.setenv("CUDABROT_AMD_NO_INTERIOR_MAP", "1")
    without_map = gpu_launches(*args, cb.CB_KERNEL_DEFAULT, projection=p)
    assert cb.lib.cb_debug_interior_map_level() == 0
    monkeypatch.delenv("CUDABROT_AMD_NO_INTERIOR_MAP")
    lockstep = gpu_launches(*args, cb.CB_KERNEL_SIMPLE, projection=p)
    assert cb.lib.cb_debug_interior_map_level() == 0
    assert (with_map[2], without_map[2], lockstep[2]) == (PRODUCT, PRODUCT, LOCKSTEP)
    for hist, cnt, _, states in (with_map, without_map):
        assert cnt["status"] == 0 and same(cnt, lockstep[1]), (cnt, lockstep[1])
        assert np.array_equal(hist, lockstep[0])
        assert np.array_equal(states, lockstep[3])
    assert lockstep[1]["status"] == 0 and lockstep[1]["never_escaped"] > 0 and lockstep[1]["increments"] > 0
    assert lockstep[1]["skipped_steps"] == 0 < without_map[1]["skipped_steps"] < with_map[1]["skipped_steps"]

    def executed(c):
        return c["iterate_steps"] + c["replay_steps"] - c["skipped_steps"]

    assert executed(with_map[1]) < executed(without_map[1]) < executed(lockstep[1])


def test_small_max_iter_does_not_consult_the_map(cb):
    """The rule of cb_draw_buddhabrot_projected: the map only where the normal product path has a LONG stage to save
    (max_iter above the 20 steps of its HEAD and MID stages at min_iter <= 16)."""
    gpu_launches(cb, 64, 64, SQUARE, 20, 5, 1024, [10], cb.CB_KERNEL_DEFAULT, projection=plot.ZR_CR)
    assert cb.lib.cb_debug_interior_map_level() == 0
    gpu_launches(cb, 64, 64, SQUARE, 21, 5, 1024, [10], cb.CB_KERNEL_DEFAULT, projection=plot.ZR_CR)
    assert cb.lib.cb_debug_interior_map_level() >= 8
    gpu_launches(cb, 64, 64, SQUARE, 500, 5, 1024, [10], cb.CB_KERNEL_DEFAULT, True, projection=plot.ZR_CR)
    assert cb.lib.cb_debug_interior_map_level() == 0  # the map is the Mandelbrot set's


# ---- 4. the renderer and the binary ---------------------------------------------------------------------------


def test_renderer_refuses_a_projection_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    good = (C.c_double * 8)(*plot.matrix(plot.ZR_CR))
    out = (C.c_double * 8)(*([7.0] * 8))
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert cb.lib.cb_renderer_set_projection(r._h, good) == 1  # a channel renderer
        assert r.projection() is None
    with cb.Renderer(dims, cb.IterationControl(100, 20), device=0, n_threads=1024) as r:
        assert cb.lib.cb_renderer_projection(r._h, out) == 0 and list(out) == [7.0] * 8
        for index in (0, 3, 7):
            p = list(plot.matrix(plot.ZR_CR))
            p[index] = float("nan") if index else float("inf")
            assert cb.lib.cb_renderer_set_projection(r._h, (C.c_double * 8)(*p)) == 1
        assert cb.lib.cb_renderer_set_projection(r._h, None) == 1
        r.set_projection(plot.ZR_CR)
        assert np.array_equal(r.projection(), np.array(plot.ZR_CR))
        assert cb.lib.cb_renderer_set_projection(r._h, good) == 1  # once
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == 1  # no focus on a projected renderer
        assert cb.lib.cb_renderer_render_passes(r._h, 1, cb.CB_KERNEL_FLAG_ANTI) == 1
        assert cb.lib.cb_renderer_render_passes(r._h, 1, cb.CB_KERNEL_FULL_ITERATE) == 1
    with cb.Renderer(dims, cb.IterationControl(100, 20), device=0, n_threads=1024) as r:
        r.render_passes(1)
        assert cb.lib.cb_renderer_set_projection(r._h, good) == 1  # after the first pass
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:
        r.set_focus(6, 4, 1)
        assert cb.lib.cb_renderer_set_projection(r._h, good) == 1  # a focused renderer


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "ship"])
def test_projected_renderer_over_several_calls(cb, ref, oracle, base, ship):
    w, h, box, m, c, threads = 300, 200, (-2.0, 1.0, -2.0, 1.0), 400, 10, 4096
    p = plot.HOLOGRAM
    variant = base | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    st = oracle.init_states(1337, 0, threads)
    want, wc = plot.draw(ref, w, h, m, c, threads, [50] * 4, projection=p, box=box, ship=ship, omp_threads=omp_threads(),
                         states=st)
    dims = cb.FractalDimensions.make(w, h, *box)
    with cb.Renderer(dims, cb.IterationControl(m, c), device=0, n_threads=threads) as r:
        r.set_projection(p)
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(3, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        states = r.read_rng_states().view(np.uint32)
        gray, mx, _ = r.grayscale_image(1.0)
    assert cnt["status"] == 0 and same(cnt, wc), (cnt, wc)
    assert np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))
    assert mx == int(want.max())
    want_gray, _, _ = cb.set_grayscale_pixels(want, 1.0)
    assert np.array_equal(gray.astype(np.uint16), want_gray)


def test_cli_plane_zr_zi_is_the_plain_command(exe, tmp_path):
    common = ["-w", "333", "-h", "77", "-m", "300", "-c", "10", "--passes", "2"]
    plain, plane = str(tmp_path / "plain.pgm"), str(tmp_path / "plane.pgm")
    assert run(exe, *common, "-o", plain).returncode == 0
    r = run(exe, *common, "-o", plane, "--plane", "zr,zi")
    assert r.returncode == 0, r.stdout + r.stderr
    with open(plain, "rb") as a, open(plane, "rb") as b:
        body = a.read()
        assert body == b.read() and any(body[20:])


@pytest.mark.parametrize("extra", [[], ["--kernel", "simple"], ["--burning-ship"]], ids=["product", "lockstep", "ship"])
def test_cli_project_image_equals_the_restatement(exe, ref, cb, oracle, tmp_path, extra):
    p = plot.HOLOGRAM.reshape(-1)
    text = ",".join(float(x).hex() for x in p[:4]) + ":" + ",".join(float(x).hex() for x in p[4:])
    out = str(tmp_path / "plot.pgm")
    r = run(exe, "--project", text, "-w", "160", "-h", "120", "-m", "300", "-c", "20", "--passes", "2", "--stats", "-o",
            out, "--tonemap", "host", *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    want, wc = plot.draw(ref, 160, 120, 300, 20, 512 * 512, [100], projection=p, ship="--burning-ship" in extra,
                         omp_threads=omp_threads())
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [float(x) for x in p]
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    gray, _, _ = cb.set_grayscale_pixels(want, 1.0)
    with open(out, "rb") as f:
        assert f.read() == oracle.encode_pgm(gray)


def test_cli_project_true_resume(exe, ref, tmp_path):
    common = ["--plane", "zr,cr", "--rotate", "zi,ci:40", "-w", "200", "-h", "100", "-m", "200", "-o", os.devnull]
    buf, side = str(tmp_path / "a.bin"), str(tmp_path / "a.rng")
    assert run(exe, "--passes", "2", "-s", buf, "--rng-state", side, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    one_buf, one_side = str(tmp_path / "b.bin"), str(tmp_path / "b.rng")
    r3 = run(exe, "--passes", "3", "-s", one_buf, "--rng-state", one_side, "--stats", *common)
    assert r3.returncode == 0
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        whole = b.read()
        assert a.read() == whole and any(whole[32:])
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()
    # the run is defined by the matrix the binary states (the host's cos and sin made it)
    p = [float.fromhex(v) for v in json.loads(r3.stderr.split("\n")[0])["projection"]]
    assert np.allclose(p, plot.rotate(plot.plane("zr", "cr"), "zi", "ci", 40.0).reshape(-1), rtol=0, atol=1e-15)
    want, _ = plot.draw(ref, 200, 100, 200, 20, 512 * 512, [150], projection=p, omp_threads=omp_threads())
    assert np.array_equal(read_state_file(buf, 100, 200), want)
