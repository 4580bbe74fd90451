"""The formula render (include/cudabrot_amd.h, "Formula step") on the GPU.  Every case three ways -- the product kernel
(cb_debug_last_draw_kernel 16), the lock-step kernel (17), the CPU restatement (tests/plot_reference.c) -- bit for bit
on histogram, generator states and every counter but skipped_steps:

  1. every formula, whole and ragged grids, two launches on the same generators;
  2. the round and chunk edges of the scheduler (max_iter around 12 and 60) and of the accept filter;
  3. the exact-periodicity early-out fires and changes nothing but the executed work;
  4. other planes on a cropped canvas;
  5. a fixed c (Julia), inside the square and on its edge;
  6. a table (palette), with zero entries, and the constant table against the render without one;
  7. everything the ABI refuses;
  8. the renderer and the binary.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import plot_harness
import plot_reference as plot
from conftest import read_state_file
from plot_harness import INVALID, SAME, SQUARE, exe, gpu_launches, omp_threads, planar_states, ref  # noqa: F401
from plot_harness import gpu_run as run
from plot_reference import demo_table

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 16, 17
CROPPED = (-1.3, 0.9, -0.7, 0.55)
C_JULIA, C_EDGE = (-0.8, 0.156), (2.0, -2.0)
NAMES = list(plot.NAMES)


def three_ways(cb, ref, oracle, name, w=64, h=64, box=SQUARE, max_iter=500, min_iter=20, threads=4096, launches=(50,),
               c=None, lut=None, projection=plot.IDENTITY):
    """Product == lock-step == restatement, without an interior map -> plot_harness.ThreeWays."""
    return plot_harness.three_ways(cb, ref, oracle, (PRODUCT, LOCKSTEP), 0, w, h, box, max_iter, min_iter, threads, launches,
                                   formula=name, c=c, lut=lut, projection=projection)


# ---- 1. every formula ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("threads,launches", [(4096, [50]), (1000, [50, 7])], ids=["whole", "ragged"])
@pytest.mark.parametrize("name", NAMES)
def test_every_formula(cb, ref, oracle, name, threads, launches):
    """64 x 64 over [-2, 2]^2, -m 500 -c 20: checked with the restatement on the CPU before the shape was fixed, every
    formula meets the condition below at both grids; none needed another -m or -c."""
    _, wc, _, _, _ = three_ways(cb, ref, oracle, name, threads=threads, launches=launches)
    assert wc["never_escaped"] > 0 and wc["too_fast"] > 0 and wc["recorded"] > 0 and wc["increments"] > wc["recorded"]
    assert wc["rejected"] == 0


# ---- 2. round and chunk edges -------------------------------------------------------------------------------------------

# rounds are 12 steps and chunks 60 (draw_rounds.h): one below, at and one above each, and two chunks
EDGES = [(m, 0) for m in (0, 1, 11, 12, 13, 59, 60, 61, 120, 121)] + [(61, 60), (61, 61), (61, 66)]


@pytest.mark.parametrize("max_iter,min_iter", EDGES, ids=["m%d_c%d" % e for e in EDGES])
@pytest.mark.parametrize("name", ["tricorn", "buffalo"])
def test_round_and_chunk_edges(cb, ref, oracle, name, max_iter, min_iter):
    _, wc, _, _, _ = three_ways(cb, ref, oracle, name, max_iter=max_iter, min_iter=min_iter, threads=1024, launches=[20])
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


@pytest.mark.parametrize("name", ["tricorn", "celtic"])
def test_early_out_changes_only_the_executed_work(cb, ref, oracle, name):
    """-m 20000 on 512 threads x 20 samples: checked with the restatement before this shape was chosen, 490 (tricorn) and
    712 (celtic) of the 10 240 samples are bit for bit at an earlier chunk boundary's point at a later one (at least 100
    are asserted again below)."""
    _, wc, product, lockstep, extra = three_ways(cb, ref, oracle, name, max_iter=20000, threads=512, launches=[20])
    assert extra["chunk_repeats"] >= 100
    assert product["skipped_steps"] > 0

    def executed(c):
        return c["iterate_steps"] - c["skipped_steps"]

    assert executed(product) < executed(lockstep) == wc["iterate_steps"]


# ---- 4. other planes -------------------------------------------------------------------------------------------------------

MATRICES = {"zr_cr": plot.ZR_CR, "hologram": plot.HOLOGRAM}


@pytest.mark.parametrize("plane", list(MATRICES))
@pytest.mark.parametrize("name", ["celtic", "perpendicular"])
def test_other_planes_on_a_cropped_canvas(cb, ref, oracle, name, plane):
    _, wc, _, _, _ = three_ways(cb, ref, oracle, name, w=333, h=77, box=CROPPED, threads=2048, projection=MATRICES[plane])
    assert 0 < wc["increments"] < wc["replay_steps"]  # points on the canvas and points off it


# ---- 5. a fixed c ------------------------------------------------------------------------------------------------------------

# at the corner of the square every start escapes within a few steps, to points outside [-2, 2]^2 (the Celtic z_1 has
# re >= 2): -c 0 and a canvas over [-7, 7]^2 there -- |z| <= 4 + 2 sqrt(2) -- so that the case does not compare empty planes
JULIA = {"inside": dict(c=C_JULIA), "edge": dict(c=C_EDGE, max_iter=100, min_iter=0, box=(-7.0, 7.0, -7.0, 7.0))}


@pytest.mark.parametrize("case", list(JULIA))
@pytest.mark.parametrize("name", ["tricorn", "celtic"])
def test_a_fixed_c_goes_into_the_same_step(cb, ref, oracle, name, case):
    want, wc, _, _, _ = three_ways(cb, ref, oracle, name, threads=1000, launches=[50, 7], projection=plot.HOLOGRAM,
                                **JULIA[case])
    assert wc["recorded"] > 0 and wc["increments"] > 0 and wc["rejected"] == 0
    # not the render that samples c
    shape = JULIA[case]
    sampled, _ = plot.draw(ref, 64, 64, shape.get("max_iter", 500), shape.get("min_iter", 20), 1000, [50, 7], formula=name,
                           projection=plot.HOLOGRAM, box=shape.get("box", SQUARE))
    assert not np.array_equal(sampled, want)


# ---- 6. a table ---------------------------------------------------------------------------------------------------------------

PALETTE = {"tricorn_sampled": dict(name="tricorn"), "perpendicular_julia": dict(name="perpendicular", c=C_JULIA)}
PLANES = {"identity": plot.IDENTITY, "zr_cr": plot.ZR_CR, "hologram": plot.HOLOGRAM}
W, H = 250, 130  # w != h: a transposed plane stride shows


@pytest.mark.parametrize("plane", list(PLANES))
@pytest.mark.parametrize("case", list(PALETTE))
def test_a_table_colours_the_orbits(cb, ref, oracle, case, plane):
    want, wc, _, _, _ = three_ways(cb, ref, oracle, w=W, h=H, threads=1000, launches=[50, 7], lut=demo_table(500),
                                projection=PLANES[plane], **PALETTE[case])
    assert wc["recorded"] > 0 and wc["increments"] > wc["recorded"]  # weighted points
    assert want[0].any() and want[1].any() and want[2].any()


@pytest.mark.parametrize("case", list(PALETTE))
def test_zero_entries_are_not_replayed(cb, ref, oracle, case):
    lut = demo_table(500)
    lut[20:40] = 0
    lut[100:] = 0
    _, wc, product, _, extra = three_ways(cb, ref, oracle, w=W, h=H, threads=1000, launches=[50, 7], lut=lut, **PALETTE[case])
    assert wc["increments"] > 0 and extra["zero_entry_steps"] > 0
    # the same run under a table without zero entries skips everything else the same way
    full = np.full(500, 0x010101, dtype=np.uint32)
    kw = PALETTE[case]
    _, cc, _, _ = gpu_launches(cb, W, H, SQUARE, 500, 20, 1000, [50, 7], cb.CB_KERNEL_FORMULA(kw["name"]), kw.get("c"), full)
    assert product["skipped_steps"] - cc["skipped_steps"] == extra["zero_entry_steps"]
    assert cc["recorded"] == wc["recorded"] and cc["replay_steps"] == wc["replay_steps"]  # zero entries still count


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("case", list(PALETTE))
def test_constant_table_equals_the_render_without_one_three_times(cb, case, base):
    kw = PALETTE[case]
    variant = base | cb.CB_KERNEL_FORMULA(kw["name"])
    shape = (W, H, SQUARE, 500, 20, 1000, [50, 7], variant, kw.get("c"))
    hist, cnt, kernel, states = gpu_launches(cb, *shape, np.full(500, 0x010101, dtype=np.uint32), plot.HOLOGRAM)
    plain, pc, plain_kernel, plain_states = gpu_launches(cb, *shape, None, plot.HOLOGRAM)
    assert kernel == plain_kernel == (LOCKSTEP if base else PRODUCT)
    assert pc["increments"] > 0
    for j in range(3):
        assert np.array_equal(hist[j], plain), j
    assert cnt["increments"] == 3 * pc["increments"]
    assert {k: cnt[k] for k in SAME if k != "increments"} == {k: pc[k] for k in SAME if k != "increments"}
    assert cnt["status"] == 0 and np.array_equal(states, plain_states)
    assert cnt["skipped_steps"] == pc["skipped_steps"]  # no entry is zero: nothing more is skipped


# ---- 7. what the ABI refuses -------------------------------------------------------------------------------------------------


def test_a_formula_is_refused_wherever_it_is_not_defined(cb):
    import torch

    dev = torch.device("cuda", 0)
    threads = 256
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    windows = (cb.IterationControl * 2)(cb.IterationControl(100, 20), cb.IterationControl(50, 5))
    mask = torch.zeros(cb.focus_mask_bytes(6), dtype=torch.uint8, device=dev)
    cells = torch.zeros(4, dtype=torch.int32, device=dev)
    d_lut = torch.full((100,), 0x010101, dtype=torch.int32, device=dev)
    bufs = plot_harness.Launches(cb, dims, threads, planes=3)
    buf, counters, states = bufs.out, bufs.counters, bufs.states
    torch.cuda.synchronize()
    before = states.cpu().numpy().copy()
    good = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    bad_matrix = (C.c_double * 8)(*([float("nan")] + list(cb.IDENTITY_PROJECTION[1:])))
    c_good = (C.c_double * 2)(*C_JULIA)
    d, b, i, s, k = C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr(), counters.data_ptr()
    lib = cb.lib

    def projected(v, p=good):
        return lib.cb_draw_buddhabrot_projected(d, b, i, p, s, threads, 5, k, v, None)

    def julia(v, c=c_good, p=good):
        return lib.cb_draw_buddhabrot_julia(d, b, i, p, c, s, threads, 5, k, v, None)

    def palette(v, c=None, lut=d_lut.data_ptr(), n=100, p=good):
        return lib.cb_draw_buddhabrot_palette(d, b, i, p, c, lut, n, s, threads, 5, k, v, None)

    # the three plotted draws: field values outside 1 .. 5, the other steps, the other flags, the other base variants
    bad_variants = [v << 16 for v in range(6, 16)]
    bad_variants += [v | cb.CB_KERNEL_SIMPLE for v in bad_variants]
    for code in range(1, 6):
        f = cb.CB_KERNEL_FORMULA(code)
        bad_variants += [f | cb.CB_KERNEL_FLAG_BURNING_SHIP, f | cb.CB_KERNEL_FLAG_ANTI, f | cb.CB_KERNEL_FLAG_DRAIN,
                         f | cb.CB_KERNEL_POWER(3), f | cb.CB_KERNEL_POWER(8), f | (1 << 12), f | cb.CB_KERNEL_TIMED,
                         f | cb.CB_KERNEL_FULL_ITERATE, f | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                         f | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI, f | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3),
                         f | cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_DRAIN, f | (1 << 20)]
    for v in bad_variants:
        assert projected(v) == INVALID, hex(v)
        assert julia(v) == INVALID, hex(v)
        assert palette(v) == INVALID and palette(v, c=c_good) == INVALID, hex(v)
    # what the projected, Julia and palette launchers refuse, with a formula as without
    nan, inf = float("nan"), float("inf")
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        v = base | cb.CB_KERNEL_FORMULA(2)
        assert projected(v, None) == INVALID and projected(v, bad_matrix) == INVALID
        assert julia(v, p=bad_matrix) == INVALID and julia(v, c=None) == INVALID
        for c in ((2.5, 0.0), (0.0, -2.0000001), (nan, 0.0), (0.0, inf)):
            assert julia(v, (C.c_double * 2)(*c)) == INVALID, c
            assert palette(v, (C.c_double * 2)(*c)) == INVALID, c
        assert palette(v, lut=None) == INVALID and palette(v, p=bad_matrix) == INVALID
        for n in (99, 101, 0):
            assert palette(v, n=n) == INVALID, n
    # every other entry point
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        for code in (1, 5):
            v = base | cb.CB_KERNEL_FORMULA(code)
            assert lib.cb_draw_buddhabrot(d, b, i, s, threads, 5, k, v, None, 0, None, None) == INVALID
            assert lib.cb_draw_buddhabrot(d, b, i, s, threads, 5, k, v | cb.CB_KERNEL_FLAG_ANTI, None, 0, None, None) == INVALID
            assert lib.cb_draw_buddhabrot_channels(d, b, windows, 2, s, threads, 5, k, v, None, 0, None, None) == INVALID
            assert lib.cb_focus_probe(d, i, s, threads, 5, 6, mask.data_ptr(), k, v, None) == INVALID
            assert lib.cb_draw_buddhabrot_focus(d, b, i, s, threads, 5, k, v, 0, None, 0, None) == INVALID
            assert lib.cb_draw_buddhabrot_focus(d, b, i, s, threads, 5, k, v, 6, cells.data_ptr(), 4, None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(mask.sum()) == 0 and int(counters.sum()) == 0
    assert np.array_equal(states.cpu().numpy(), before)
    # no threads or no samples: nothing launched, success
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        v = base | cb.CB_KERNEL_FORMULA(3)
        assert lib.cb_draw_buddhabrot_projected(d, b, i, good, s, threads, 0, k, v, None) == 0
        assert lib.cb_draw_buddhabrot_julia(d, b, i, good, c_good, s, 0, 5, k, v, None) == 0
        assert lib.cb_draw_buddhabrot_palette(d, b, i, good, None, d_lut.data_ptr(), 100, s, threads, 0, k, v, None) == 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int(counters.sum()) == 0 and np.array_equal(states.cpu().numpy(), before)


def test_renderer_refuses_a_formula_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    tricorn = cb.CB_KERNEL_FORMULA("tricorn")
    with cb.Renderer(dims, it, device=0, n_threads=256) as r:  # a plain renderer
        fresh = r.read_rng_states().copy()
        for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
            assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, tricorn | base) == INVALID
            assert cb.lib.cb_renderer_render_passes(r._h, 1, tricorn | base) == INVALID
        assert r.focus_cells() == (0, 0)
        assert int(r.read_histogram().sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
        r.set_projection(cb.IDENTITY_PROJECTION)  # still possible: nothing was rendered
        for variant in (6 << 16, 15 << 16, tricorn | cb.CB_KERNEL_FLAG_BURNING_SHIP, tricorn | cb.CB_KERNEL_FLAG_ANTI,
                        tricorn | cb.CB_KERNEL_FLAG_DRAIN, tricorn | cb.CB_KERNEL_POWER(3), tricorn | cb.CB_KERNEL_TIMED):
            assert cb.lib.cb_renderer_render_passes(r._h, 1, variant) == INVALID
        assert int(r.read_histogram().sum()) == 0 and r.read_counters().as_dict()["samples"] == 0
        assert np.array_equal(r.read_rng_states(), fresh)
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=256) as r:  # a channel renderer
        assert cb.lib.cb_renderer_render_passes(r._h, 1, tricorn) == INVALID
        assert int(r.read_histogram().sum()) == 0
    focus_box = cb.FractalDimensions.make(64, 64, -0.2, 0.0, -0.9, -0.7)
    with cb.Renderer(focus_box, cb.IterationControl(300, 20), device=0, n_threads=4096) as r:  # a focused renderer
        r.set_focus(6, 4, 1)
        assert cb.lib.cb_renderer_render_passes(r._h, 1, tricorn) == INVALID
        assert cb.lib.cb_renderer_render_passes(r._h, 1, tricorn | cb.CB_KERNEL_SIMPLE) == INVALID
        assert int(r.read_histogram().sum()) == 0 and r.read_counters().as_dict()["samples"] == 0


# ---- 8. the renderer and the binary -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("kind", ["projected", "julia", "palette"])
def test_renderer_passes_equal_the_restatement(cb, ref, oracle, base, kind):
    w, h, m, mn, threads, name = 64, 48, 300, 10, 1000, "celtic-tricorn"
    c = C_JULIA if kind == "julia" else None
    lut = None
    if kind == "palette":
        lut = demo_table(m)
        lut[50:70] = 0
    st = oracle.init_states(1337, 0, threads)
    want, wc = plot.draw(ref, w, h, m, mn, threads, [50] * 3, formula=name, c=c, lut=lut, projection=plot.HOLOGRAM,
                         omp_threads=omp_threads(), states=st)
    variant = base | cb.CB_KERNEL_FORMULA(name)
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(m, mn), device=0, n_threads=threads) as r:
        if kind == "julia":
            r.set_julia(c, plot.HOLOGRAM)
        else:
            r.set_projection(plot.HOLOGRAM)
        if kind == "palette":
            r.set_palette(lut)
        r.prepare(variant)  # must not fail
        r.render_passes(1, variant)
        r.finish()
        r.render_passes(2, variant)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        assert cb.lib.cb_renderer_interior_map_level(r._h) == 0
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        states = r.read_rng_states().view(np.uint32)
    assert wc["recorded"] > 100 and wc["increments"] > 100  # not empty
    assert cnt["status"] == 0 and {k: cnt[k] for k in SAME} == wc, (cnt, wc)
    assert hist.shape == want.shape and np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))


SHAPE = ["-w", "64", "-h", "64", "-m", "100", "-c", "20"]


def test_cli_formula_image_stats_and_resume(exe, ref, cb, oracle, tmp_path):
    common = ["--formula", "tricorn", *SHAPE]
    one_buf, one_side, one_pgm = str(tmp_path / "one.bin"), str(tmp_path / "one.rng"), str(tmp_path / "one.pgm")
    r = run(exe, "--passes", "2", "-s", one_buf, "--rng-state", one_side, "--stats", "-o", one_pgm, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert [float.fromhex(v) for v in json.loads(lines[0])["projection"]] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert json.loads(lines[1]) == {"formula": "tricorn"}
    want, wc = plot.draw(ref, 64, 64, 100, 20, 512 * 512, [100], formula="tricorn", omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc
    assert wc["increments"] > 100000
    gray, _, _ = cb.set_grayscale_pixels(want, 1.0)
    with open(one_pgm, "rb") as f:
        assert f.read() == oracle.encode_pgm(gray)  # the header, then the values byte-swapped
    assert np.array_equal(read_state_file(one_buf, 64, 64), want)
    # one pass, the two files written, then one more pass on them: the same run
    buf, side = str(tmp_path / "two.bin"), str(tmp_path / "two.rng")
    assert run(exe, "--passes", "1", "-s", buf, "--rng-state", side, "-o", os.devnull, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, "-o", str(tmp_path / "two.pgm"), *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 1 passes." in r2.stdout, r2.stdout
    for a, b in ((buf, one_buf), (side, one_side), (str(tmp_path / "two.pgm"), one_pgm)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), a


def test_cli_formula_with_a_palette_writes_the_matching_ppm(exe, ref, cb, tmp_path):
    stops_text, stops = "20:000030,60:ff8000,99:ffffff", [(20, 0x00, 0x00, 0x30), (60, 0xFF, 0x80, 0x00), (99, 0xFF, 0xFF, 0xFF)]
    lut = cb.palette_from_stops(stops, 100)
    ppm = str(tmp_path / "t.ppm")
    r = run(exe, "--formula", "tricorn", "--palette", stops_text, "--passes", "1", "-g", "2.2", "--stats", "-o", ppm, *SHAPE)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.strip().split("\n")
    assert json.loads(lines[1]) == {"formula": "tricorn"} and "palette" in json.loads(lines[2])
    want, wc = plot.draw(ref, 64, 64, 100, 20, 512 * 512, [50], formula="tricorn", lut=lut, omp_threads=omp_threads())
    stats = json.loads(lines[-1])
    assert stats["status"] == 0 and {k: stats[k] for k in SAME} == wc and wc["recorded"] > 10000
    gray, _, _ = cb.set_grayscale_pixels(want.reshape(3 * 64, 64), 2.2)  # "Palette render", Image: one common maximum
    body = np.ascontiguousarray(gray.reshape(3, 64, 64).transpose(1, 2, 0)).astype(">u2")
    with open(ppm, "rb") as f:
        data = f.read()
    header = b"P6\n64 64\n65535\n"
    assert data[:len(header)] == header and data[len(header):] == body.tobytes()
