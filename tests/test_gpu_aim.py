"""The aimed render (include/cudabrot_amd.h, "Aimed render") on the GPU, bit for bit on mask, list,
histogram, generator states and counters (skipped_steps as the un-aimed suites treat it):

  1. the issue's table: product kernels (30) == lock-step kernel (31) == CPU restatement (tests/aim_reference.c), and every
     case reaches the paths it is there for -- asserted from the restatement;
  2. anchor 1: with no list the aimed kernels are the un-aimed kernels (8/9 .. 16/17, 26/27), every step, source and kind;
  3. anchor 2: with the identity matrix, the reference's step, a sampled c and escaping orbits the probe is cb_focus_probe
     and the draw cb_draw_buddhabrot_focus;
  4. the interior map on and off, launches that add up, the refusals, a probe that marks nothing;
  5. the renderer: cb_renderer_set_aim on every starting renderer, an aimed renderer against every setter,
     CB_ERROR_AIM_EMPTY, the renderer against the entry points, a wrong step;
  6. the binary against the API.

Common shape (aim_reference.py): 64 x 48, 1000 threads, seed 1337, level 6, dilate 1, M = 500, -c 20, the probe as 3 + 13
samples per thread, the draw as 3 + 50 + 1.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import aim_reference as aim
import plot_reference as plot
from aim_harness import BASES, LOCKSTEP, PRODUCT, aref, bits, gpu_draw, gpu_probe, source_args, three_ways, variant  # noqa: F401
from conftest import read_state_file
from device_launches import SAME, Launches, gpu_run as run
from plot_harness import INVALID, exe, variant_of  # noqa: F401 (exe: a fixture)
from test_aim_host import STEP_IDS, STEPS
from test_gpu_renderer_kinds import getters, library_planes, make

pytestmark = pytest.mark.gpu


# ---- 1. the table ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(aim.CASES))
def test_three_ways_on_the_table(cb, aref, oracle, name):  # noqa: F811
    case = aim.CASES[name]
    s = aim.shape_of(case)
    got = three_ways(cb, aref, oracle, **case)
    (pc, pex), (dc, dex) = got["probe"], got["draw"]
    print(name, "marked", bits(got["mask"]), "listed", len(got["cells"]), "probe", pc, pex, "draw", dc, dex)
    # from the restatement: the case is what the model says and reaches its paths
    assert (bits(got["mask"]), len(got["cells"])) == (case["marked"], case["listed"])
    assert 0 < len(got["cells"]) < (4 << s["level"]) ** 2
    assert dex["in_canvas"] > 0 and dex["off_canvas"] > 0  # every window is a crop
    if "plotted" in case:
        assert dc["recorded"] == case["plotted"]
    if "cycles" in case:
        assert (dex["cycles"], dex["no_cycle"]) == (case["cycles"], case["no_cycle"])
    if s["bounded"]:
        assert dex["both_weights"] > 0
        assert got["product"]["skipped_steps"] > 0  # cycles are replayed compressed
        if s["c"] is None:
            assert dex["cycles"] > 0 and dex["no_cycle"] > 0
    else:
        assert dc["never_escaped"] > 0 and (dc["rejected"] > 0) == aim.rejects(s)
        assert cb.lib.cb_debug_interior_map_level() == 0  # the last launch was the lock-step kernel's: no map


# ---- 2. anchor 1: no list, no mask -> the un-aimed kernels -----------------------------------------------------------------

def unaimed_draw(cb, lockstep, **kw):
    s = aim.shape_of(kw)
    bufs = Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"])
    args = source_args(cb, s)
    del args["bounded"]
    if s["bounded"]:
        entry = cb.draw_buddhabrot_bounded
    elif s["c"] is not None:
        entry = cb.draw_buddhabrot_julia
    else:
        entry = cb.draw_buddhabrot_projected
        del args["julia_c"]
    return bufs.launches(entry, s["draw"], variant(cb, lockstep, s), **args).read()


@pytest.mark.parametrize("step", STEPS, ids=STEP_IDS)
def test_with_no_list_the_aimed_kernels_are_the_unaimed_kernels(cb, step):
    for bounded in (False, True):
        for c in (None, (0.1, 0.1)):
            # -c 2: the Julia set of this c has escaping orbits under every step, all of them short
            kw = dict(step, bounded=bounded, c=c, projection=plot.HOLOGRAM, box=(-1.2, 0.9, -0.8, 1.1), min_iter=2)
            for lockstep, kernel in BASES:
                hist, cnt, launched, states = gpu_draw(cb, lockstep, None, **kw)
                level = cb.lib.cb_debug_interior_map_level()
                want, wc, other, wstates = unaimed_draw(cb, lockstep, **kw)
                what = (step, bounded, c, kernel)
                assert launched == kernel and other not in (PRODUCT, LOCKSTEP) and other % 2 == lockstep, what
                assert cnt["status"] == 0 and cnt == wc, (what, cnt, wc)  # every counter, skipped_steps too
                assert np.array_equal(hist, want) and np.array_equal(states, wstates), what
                assert cnt["recorded"] > 0 and int(hist.sum()) == cnt["increments"] > 0, what
                assert level == cb.lib.cb_debug_interior_map_level(), what  # the map by the un-aimed render's own rule
                mandelbrot = not step and not bounded and c is None and not lockstep
                assert (level > 0) == mandelbrot, what


# ---- 3. anchor 2: the identity case is the focused render -----------------------------------------------------------------


@pytest.mark.parametrize("ship", [False, True], ids=["reference", "ship"])
def test_the_identity_case_is_the_focused_render(cb, ship):
    case = dict(aim.CASES["ship_identity" if ship else "identity_body"])
    s = aim.shape_of(case)
    dims, it = cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), cb.IterationControl(s["max_iter"], s["min_iter"])
    flag = cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0
    cells = None
    for lockstep, kernel in BASES:
        base = (cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT) | flag
        mask, pc, launched, pstates = gpu_probe(cb, lockstep, **case)
        f = Launches(cb, dims, s["threads"], words=aim.mask_words(s["level"]))
        fmask, fpc, fkernel, fstates = f.launches(cb.focus_probe, s["probe"], base, iterations=it, level=s["level"]).read()
        assert (launched, fkernel) == (kernel, 7 if lockstep else 6)
        assert np.array_equal(mask, fmask) and np.array_equal(pstates, fstates) and bits(mask) == case["marked"]
        assert {k: pc[k] for k in SAME} == {k: fpc[k] for k in SAME}
        cells = cb.focus_cells(s["level"], mask, s["dilate"])
        assert len(cells) == case["listed"]
        hist, dc, launched, dstates = gpu_draw(cb, lockstep, cells, **case)
        f = Launches(cb, dims, s["threads"], tables={"cells": cells})
        fhist, fdc, fkernel, fdstates = f.launches(cb.draw_buddhabrot_focus, s["draw"], base, iterations=it, level=s["level"],
                                                   d_cells=f.tables["cells"].data_ptr(), n_cells=len(cells)).read()
        assert (launched, fkernel) == (kernel, 7 if lockstep else 6)
        assert np.array_equal(hist, fhist) and np.array_equal(dstates, fdstates)
        assert {k: dc[k] for k in SAME} == {k: fdc[k] for k in SAME} and dc["recorded"] == case["plotted"]
        if not lockstep and not ship:  # the map level apart: the aimed draw has the interior map, kernel 6 has none
            assert dc["skipped_steps"] >= fdc["skipped_steps"]


# ---- 4. the map, sums, refusals, nothing marked -----------------------------------------------------------------------------


def test_the_interior_map_changes_the_work_and_nothing_else(cb, monkeypatch):
    # the whole set on the canvas, M = 2000: marked cells are listed, and an unmarked interior sample costs a period search
    case = dict(box=(-2.0, 0.5, -1.25, 1.25), max_iter=2000, level=5)
    mask, pc, _, pstates = gpu_probe(cb, 0, **case)
    assert cb.lib.cb_debug_interior_map_level() >= 8
    cells = cb.focus_cells(5, mask, 1)
    with_map = gpu_draw(cb, 0, cells, **case)
    assert cb.lib.cb_debug_interior_map_level() >= 8
    monkeypatch.setenv("CUDABROT_AMD_NO_INTERIOR_MAP", "1")
    mask0, pc0, _, pstates0 = gpu_probe(cb, 0, **case)
    assert cb.lib.cb_debug_interior_map_level() == 0
    without = gpu_draw(cb, 0, cells, **case)
    assert cb.lib.cb_debug_interior_map_level() == 0
    monkeypatch.delenv("CUDABROT_AMD_NO_INTERIOR_MAP")
    assert np.array_equal(mask, mask0) and np.array_equal(pstates, pstates0)
    assert {k: pc[k] for k in SAME} == {k: pc0[k] for k in SAME} and pc["skipped_steps"] > pc0["skipped_steps"]
    (h1, c1, k1, s1), (h0, c0, k0, s0) = with_map, without
    assert k1 == k0 == PRODUCT and np.array_equal(h1, h0) and np.array_equal(s1, s0)
    assert {k: c1[k] for k in SAME} == {k: c0[k] for k in SAME} and c1["never_escaped"] > 0
    executed = [c["iterate_steps"] + c["replay_steps"] - c["skipped_steps"] for c in (c1, c0)]
    print("executed steps with the map", executed[0], "without", executed[1])
    assert executed[0] < executed[1]


@pytest.mark.parametrize("name", ["plane_zr_cr", "bounded_julia_130"])
def test_consecutive_launches_equal_one_launch_of_the_sum(cb, name):
    case = aim.CASES[name]
    mask, pc, _, pstates = gpu_probe(cb, 0, **case)
    one_mask, one_pc, _, one_states = gpu_probe(cb, 0, **dict(case, probe=(16,)))
    assert np.array_equal(mask, one_mask) and np.array_equal(pstates, one_states) and pc == one_pc
    cells = cb.focus_cells(aim.LEVEL, mask, aim.DILATE)
    hist, dc, _, states = gpu_draw(cb, 0, cells, **case)
    one, one_dc, _, one_states = gpu_draw(cb, 0, cells, **dict(case, draw=(54,)))
    assert np.array_equal(hist, one) and np.array_equal(states, one_states)
    assert {k: dc[k] for k in SAME} == {k: one_dc[k] for k in SAME}


def test_entry_points_refuse_what_they_do_not_define_with_nothing_written(cb):
    import torch

    dims, it = cb.FractalDimensions.make(64, 48), cb.IterationControl(100, 20)
    no_pixels = cb.FractalDimensions.make(64, 48)
    no_pixels.w = 0
    threads = 256
    bufs = Launches(cb, dims, threads, words=aim.mask_words(6), tables={"cells": np.arange(7, dtype=np.uint32)})
    hist = torch.zeros(64 * 48, dtype=torch.int64, device=bufs.dev)
    fresh = bufs.states.clone()
    p = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_p = (C.c_double * 8)(*([float("nan")] + [0.0] * 7))
    c = (C.c_double * 2)(-1.0, 0.0)
    bad_c = (C.c_double * 2)(2.5, 0.0)
    st, mask, cnt, cells = bufs.states.data_ptr(), bufs.out.data_ptr(), bufs.counters.data_ptr(), bufs.tables["cells"].data_ptr()
    D, S = cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE

    def probe(dims_=dims, it_=it, p_=p, c_=None, bounded=0, st_=st, level=6, mask_=mask, v=D):
        return cb.lib.cb_aim_probe(C.byref(dims_) if dims_ else None, C.byref(it_) if it_ else None, p_, c_, bounded, st_,
                                   threads, 5, level, mask_, cnt, v, bufs.stream)

    def draw(dims_=dims, hist_=None, it_=it, p_=p, c_=None, bounded=0, st_=st, v=D, level=6, cells_=cells, n=7):
        return cb.lib.cb_draw_buddhabrot_aimed(C.byref(dims_) if dims_ else None, hist.data_ptr() if hist_ is None else hist_,
                                               C.byref(it_) if it_ else None, p_, c_, bounded, st_, threads, 5, cnt, v, level,
                                               cells_, n, bufs.stream)

    bad_variants = (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED,
                    cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP, 2 << 12, 9 << 12,  # (degrees 2 and 9)
                    6 << 16, cb.CB_KERNEL_FORMULA(1) | cb.CB_KERNEL_POWER(3),  # (formula code 6)
                    cb.CB_KERNEL_FORMULA(2) | cb.CB_KERNEL_FLAG_BURNING_SHIP)
    refused = [
        probe(dims_=None), probe(it_=None), probe(p_=None), probe(p_=bad_p), probe(c_=bad_c), probe(st_=None),
        probe(mask_=None), probe(level=3), probe(level=11), probe(level=0), probe(dims_=no_pixels),
        draw(dims_=None), draw(hist_=0), draw(it_=None), draw(p_=None), draw(p_=bad_p), draw(c_=bad_c), draw(st_=None),
        draw(dims_=no_pixels), draw(level=3), draw(level=11), draw(level=0), draw(cells_=None), draw(n=0),
        draw(level=0, cells_=None, n=7), draw(level=6, cells_=None, n=0), draw(level=0, n=0),
    ]
    for bounded in (0, 1):
        for v in bad_variants:
            refused += [probe(bounded=bounded, v=v), probe(bounded=bounded, c_=c, v=v | S), draw(bounded=bounded, v=v),
                        draw(bounded=bounded, c_=c, v=v | S), draw(bounded=bounded, v=v, level=0, cells_=None, n=0)]
    assert refused == [INVALID] * len(refused), refused
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0 and int(bufs.out.abs().sum()) == 0 and int(bufs.counters.abs().sum()) == 0
    assert torch.equal(bufs.states, fresh)
    # and what they do define goes through on the same buffers
    assert probe() == 0 and probe(bounded=1, c_=c, v=S) == 0 and draw() == 0 and draw(level=0, cells_=None, n=0) == 0
    torch.cuda.synchronize()
    assert int(bufs.counters.cpu().numpy().view(np.uint64)[0]) == 4 * 5 * threads


def test_a_probe_that_marks_nothing_leaves_the_mask_zero(cb, aref, oracle):  # noqa: F811
    case = {k: v for k, v in aim.CASES["bounded_zr_cr"].items() if k not in aim.MODEL_KEYS}
    got = three_ways(cb, aref, oracle, **dict(case, box=(-2.0, 2.0, -1.79, -1.74)))
    pc, pex = got["probe"]
    assert not got["mask"].any() and len(got["cells"]) == 0 and "hist" not in got
    assert pc["recorded"] == 0 and pc["never_escaped"] > 0 and pc["replay_steps"] == 500 * pc["never_escaped"]


# ---- 5. the renderer ------------------------------------------------------------------------------------------------------

# cb_renderer_set_aim on the starting renderers of tests/test_gpu_renderer_kinds.py: 1 accepted, 0 refused -- literal data.
# The 16 x 16 canvas of its plain renderers is the whole plane, so every probe marks cells.
AIM_COLUMN = {
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


@pytest.mark.parametrize("name", list(AIM_COLUMN))
def test_set_aim_on_every_starting_renderer(cb, name):
    accepted = AIM_COLUMN[name]
    with make(cb, name, name == "focused") as r:
        h, w = r.dims.h, r.dims.w
        before, hist = getters(r), r.read_histogram()
        assert r.aim_cells() == (0, 0)
        code = cb.lib.cb_renderer_set_aim(r._h, 6, 2, 1, 0)
        if not accepted:
            assert code == INVALID and r.aim_cells() == (0, 0)
            assert getters(r) == before
            after = r.read_histogram()
            assert after.shape == hist.shape and np.array_equal(after, hist)
            assert library_planes(cb, r) == (hist.shape[0] if hist.ndim == 3 else 1)
            return
        assert code == 0
        listed, total = r.aim_cells()
        assert 0 < listed <= total == 256 * 256
        now = getters(r)  # the source of c stays; a plain renderer gains the identity; focus_cells stays (0, 0)
        assert now[1:] == before[1:] and np.ravel(now[0]).tolist() == list(cb.IDENTITY_PROJECTION) and now[-1] == (0, 0)
        assert r.read_histogram().shape == (h, w) and library_planes(cb, r) == 1 and not r.bounded()
        assert cb.lib.cb_renderer_set_aim(r._h, 6, 2, 1, 0) == INVALID  # once
        r.render_passes(1)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT
        cnt = r.read_counters().as_dict()
        assert int(r.read_histogram().sum()) == cnt["increments"] > 0 and cnt["status"] == 0 and cnt["recorded"] > 0
        assert cnt["samples"] == 50 * 256  # the probe ran on generators and counters of its own


def test_an_aimed_renderer_refuses_all_eleven_setters(cb):
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
        "period_palette": lambda r: cb.lib.cb_renderer_set_period_palette(r._h, slice_table.ctypes.data, 4, 0.0),
        "aim": lambda r: cb.lib.cb_renderer_set_aim(r._h, 6, 2, 1, 0),
    }
    for start in ("plain", "projected", "julia", "bounded", "julia bounded"):
        with cb.Renderer(dims, it, device=0, n_threads=256) as r:
            if start == "projected":
                r.set_projection(plot.ZR_CR)
            elif start.startswith("julia"):  # a c with bounded orbits for the bounded kind, with slow escapes for the other
                r.set_julia((0.1, 0.1) if start.endswith("bounded") else (-0.8, 0.156), plot.ZR_CR)
            if start.endswith("bounded"):
                r.set_bounded()
            cells = r.set_aim(6, 2, 1)
            assert cells[0] > 0 and r.bounded() == start.endswith("bounded")
            before = getters(r)
            fresh = r.read_rng_states().copy()
            for name, setter in setters.items():
                assert setter(r) == INVALID, (start, name)
                assert getters(r) == before and r.aim_cells() == cells, (start, name)
            # render_passes takes what the entry point takes, and only the probe's step
            for v in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED,
                      cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP, cb.CB_KERNEL_FORMULA(1), cb.CB_KERNEL_POWER(3),
                      cb.CB_KERNEL_FLAG_BURNING_SHIP, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP):
                assert cb.lib.cb_renderer_render_passes(r._h, 1, v) == INVALID, (start, v)
            hist = r.read_histogram()
            assert hist.shape == (16, 16) and int(hist.sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
            assert np.array_equal(r.read_rng_states(), fresh)
            r.render_passes(1, cb.CB_KERNEL_SIMPLE)  # the base may change, the step may not
            assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP
            assert int(r.read_histogram().sum()) == r.read_counters().as_dict()["increments"] > 0


def test_an_empty_probe_is_its_own_error_and_leaves_the_renderer_usable(cb):
    dims = cb.FractalDimensions.make(16, 16, 5.0, 6.0, -0.5, 0.5)  # nothing reaches u in [5, 6]
    with cb.Renderer(dims, cb.IterationControl(100, 20), device=0, n_threads=256) as r:
        r.set_projection(plot.ZR_CR)
        before = getters(r)
        with pytest.raises(cb.CudabrotError) as e:
            r.set_aim(6, 2, 1)
        assert e.value.code == cb.CB_ERROR_AIM_EMPTY == 100003 and "aim probe marked no cell" in str(e.value)
        assert getters(r) == before and r.aim_cells() == (0, 0)
        r.render_passes(1)  # still the projected renderer it was, on untouched generators
        assert cb.lib.cb_debug_last_draw_kernel() == 8
        cnt = r.read_counters().as_dict()
        assert cnt["samples"] == 50 * 256 and cnt["recorded"] > 0 and cnt["increments"] == 0


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("name", ["plane_zr_cr", "bounded_zr_cr", "bounded_julia_130", "power3_rotated", "ship_identity"])
def test_renderer_against_the_entry_points_on_identical_passes(cb, base, name):
    case = dict(aim.CASES[name], probe=(100,), draw=(50, 100))  # two probe passes fused; one pass, then two fused
    s = aim.shape_of(case)
    mask, _, _, _ = gpu_probe(cb, base, **case)
    cells = cb.focus_cells(s["level"], mask, s["dilate"])
    want, wc, kernel, states = gpu_draw(cb, base, cells, **case)
    v = variant(cb, base, s)
    dims = cb.FractalDimensions.make(s["w"], s["h"], *s["box"])
    with cb.Renderer(dims, cb.IterationControl(s["max_iter"], s["min_iter"]), device=0, n_threads=s["threads"]) as r:
        if s["c"] is not None:
            r.set_julia(s["c"], s["projection"])
        elif name != "ship_identity":  # (that one alone: the plain renderer gains the identity)
            r.set_projection(s["projection"])
        if s["bounded"]:
            r.set_bounded()
        assert r.set_aim(s["level"], 2, s["dilate"], v) == (len(cells), (4 << s["level"]) ** 2)
        assert r.focus_cells() == (0, 0)
        r.render_passes(1, v)
        r.render_passes(2, v)
        assert cb.lib.cb_debug_last_draw_kernel() == kernel
        assert np.array_equal(r.read_histogram(), want)
        cnt = r.read_counters().as_dict()
        assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == {k: wc[k] for k in SAME}
        assert np.array_equal(r.read_rng_states().view(np.uint32).reshape(-1), states)
        if not s["bounded"] and name == "plane_zr_cr" and not base:
            assert cb.lib.cb_renderer_interior_map_level(r._h) >= 8


# ---- 6. the binary --------------------------------------------------------------------------------------------------------

CLI_W, CLI_H, CLI_MAX, CLI_MIN = 64, 48, 130, 10
CLI_AIM = ["--aim-level", "6", "--aim-probe", "2", "--aim-dilate", "1"]
CLI_RUNS = {
    # flags, window, what the API is given: bounded, c, projection, variant
    "bounded_zr_cr": (["--bounded", "--plane", "zr,cr"], (-2.0, 2.0, -1.5, -1.25), True, None, plot.ZR_CR, 0),
    "julia": (["--julia", "-0.123,0.745"], (0.2, 0.7, 0.2, 0.7), False, (-0.123, 0.745), None, 0),
    "alone": ([], (-0.2, 0.0, -0.9, -0.7), False, None, None, 0),
    "tricorn": (["--formula", "tricorn", "--bounded", "--plane", "zr,cr"], (-2.0, 2.0, -1.25, -0.75), True, None, plot.ZR_CR,
                "tricorn"),
}


def api_render(cb, name, passes, base=0):
    """What the binary's run is: a renderer of its default threads and seed -> (hist, counters, (listed, total))."""
    flags, box, bounded, c, projection, v = CLI_RUNS[name]
    v = base | (cb.CB_KERNEL_FORMULA(1) if v == "tricorn" else 0)
    dims = cb.FractalDimensions.make(CLI_W, CLI_H, *box)
    with cb.Renderer(dims, cb.IterationControl(CLI_MAX, CLI_MIN), device=0) as r:
        if c is not None:
            r.set_julia(c, projection)
        elif projection is not None:
            r.set_projection(projection)
        if bounded:
            r.set_bounded()
        cells = r.set_aim(6, 2, 1, v)
        for p in passes:
            r.render_passes(p, v)
        return r.read_histogram(), r.read_counters().as_dict(), cells


def cli_flags(name):
    flags, box = CLI_RUNS[name][:2]
    window = ["--min-real", repr(box[0]), "--max-real", repr(box[1]), "--min-imag", repr(box[2]), "--max-imag", repr(box[3])]
    return flags + CLI_AIM + ["-w", str(CLI_W), "-h", str(CLI_H), "-m", str(CLI_MAX), "-c", str(CLI_MIN), "-o", os.devnull] + window


KEYS = SAME + ("skipped_steps",)


@pytest.mark.parametrize("name", list(CLI_RUNS))
def test_cli_aim_equals_the_api_and_resumes(cb, exe, tmp_path, name):  # noqa: F811
    want, wc, (listed, total) = api_render(cb, name, [4])
    assert wc["recorded"] > 0 and wc["increments"] > 0 and 0 < listed < total
    common = cli_flags(name)
    one_buf, one_side = str(tmp_path / "one.bin"), str(tmp_path / "one.rng")
    r = run(exe, "--passes", "4", "-s", one_buf, "--rng-state", one_side, "--stats", *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Aim: sampling %d of %d cells of side 2^-6 (2 probe passes, dilated by 1)." % (listed, total) in r.stdout.split("\n")
    lines = r.stderr.strip().split("\n")
    assert {"aim": {"level": 6, "probe": 2, "dilate": 1}} in [json.loads(line) for line in lines[1:-1]]
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in KEYS} == {k: wc[k] for k in KEYS}
    assert (stats["aim_cells"], stats["aim_total"]) == (listed, total) and "focus_cells" not in stats
    assert stats["aim_fraction"] == pytest.approx(listed / total, rel=1e-8)
    assert np.array_equal(read_state_file(one_buf, CLI_H, CLI_W), want)
    # two passes, the two files written, then two more on them: the list is rebuilt, the sample stream continues
    buf, side = str(tmp_path / "two.bin"), str(tmp_path / "two.rng")
    assert run(exe, "--passes", "2", "-s", buf, "--rng-state", side, *common).returncode == 0
    r2 = run(exe, "--passes", "2", "-s", buf, "--rng-state", side, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        assert a.read() == b.read()
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()


def test_cli_aim_raw_format_and_the_lock_step_kernel(cb, exe, tmp_path):  # noqa: F811
    name = "bounded_zr_cr"
    want, wc, _ = api_render(cb, name, [2])
    common = cli_flags(name)
    raw, side = str(tmp_path / "raw.bin"), str(tmp_path / "raw.rng")
    assert run(exe, "--passes", "1", "-s", raw, "--state-format", "raw", "--rng-state", side, *common).returncode == 0
    r = run(exe, "--passes", "1", "-s", raw, "--state-format", "raw", "--rng-state", side, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(raw, dtype=np.uint32).reshape(CLI_H, CLI_W), want)
    simple = str(tmp_path / "simple.bin")
    r3 = run(exe, "--kernel", "simple", "--passes", "2", "-s", simple, "--stats", *common)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    stats = json.loads(r3.stderr.strip().split("\n")[-1])
    assert {k: stats[k] for k in SAME} == {k: wc[k] for k in SAME} and stats["skipped_steps"] == 0 < wc["skipped_steps"]
    assert np.array_equal(read_state_file(simple, CLI_H, CLI_W), want)
    lock, lc, _ = api_render(cb, name, [2], cb.CB_KERNEL_SIMPLE)
    assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP and lc["skipped_steps"] == 0 and np.array_equal(lock, want)


def test_cli_aim_with_an_empty_list_exits_1_without_an_image(exe, tmp_path):  # noqa: F811
    out = str(tmp_path / "none.pgm")
    r = run(exe, "--aim", "--aim-probe", "2", "--plane", "zr,cr", "--max-real", "6", "--min-real", "5", "-w", "16", "-h", "16",
            "--passes", "1", "-o", out)
    assert r.returncode == 1
    assert "Aim: no sample of the 2 probe passes reaches the canvas; nothing to render." in r.stdout.split("\n")
    assert not os.path.exists(out)
