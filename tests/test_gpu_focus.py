"""The focused render (include/cudabrot_amd.h, "Focused render") on the GPU, bit for bit on histogram, mask, generator
states and counters (all but skipped_steps):

  1. the focus kernels with the uniform source against the oracle (a normal render through draw_focus.hip);
  2. the probe against the CPU restatement (tests/focus_reference.c): mask words and counters;
  3. the focused draw: lock-step kernel against the restatement, product kernel against lock-step, on probed and planted
     cell lists, and at the max_iter that put the exact-periodicity early-out on, before and after a chunk boundary;
  4. the renderer (set_focus, resume) and the CLI against the restatement;
  5. what the feature is for: in-canvas increments per sample of a focused render against a normal one.
"""

import ctypes as C
import os

import numpy as np
import pytest

import focus_reference as focus
from device_launches import SAME, SQUARE, Launches, assert_same, gpu_run as run, omp_threads, planar_states  # noqa: F401
from plot_harness import exe, write_states  # noqa: F401 (exe: a fixture)

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 6, 7
PROBE_LAUNCHES = [50] * 8  # 8 reference passes of 4096 threads: 1.6e6 samples


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return focus.load(tmp_path_factory.mktemp("focus_ref"))


def gpu_launches(cb, w, h, box, max_iter, min_iter, threads, launches, base, ship=False, level=0, cell_list=None,
                 probe=False, states=None, guard=0):
    """`launches` (samples per thread each) on fresh generators (seed 1337, subsequences [0, threads)), or on the given
    oracle `states` written over them (they are left as they were) -> (u64 hist [h, w] or, probe=True, the mask's u32 words,
    with `guard` words allocated before and after them and read back too; counters dict; cb_debug_last_draw_kernel;
    generator states as u32 planes)."""
    seq = Launches(cb, cb.FractalDimensions.make(w, h, *box), threads,
                   words=focus.mask_words(level) + 2 * guard if probe else None,
                   tables={} if cell_list is None else {"cells": cell_list})
    if states is not None:
        write_states(seq, states)
    variant = base | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    args = dict(iterations=cb.IterationControl(max_iter, min_iter), level=level)
    if not probe and cell_list is not None:
        args.update(d_cells=seq.tables["cells"].data_ptr(), n_cells=seq.tables["cells"].numel())

    def probe_entry(d_hist, **a):  # the scaffolding's output buffer is the mask, between its guards
        cb.focus_probe(d_mask=d_hist + 4 * guard, **a)

    return seq.launches(probe_entry if probe else cb.draw_buddhabrot_focus, launches, variant, **args).read()


# ---- 1. the uniform source: a normal render through the focus kernels -------------------------------------------------

CANVASES = {
    "square": (256, 256, SQUARE, False),
    "zoom": (300, 200, (-1.9, -0.7, -0.45, 0.35), False),  # deltas 0.004, 0.004: not powers of two
    "ship": (256, 256, SQUARE, True),
}


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
@pytest.mark.parametrize("threads", [4096, 4000])
@pytest.mark.parametrize("max_iter,min_iter", [(100, 20), (1000, 20), (2000, 200)])
@pytest.mark.parametrize("canvas", list(CANVASES))
def test_uniform_source_equals_the_oracle(cb, oracle, canvas, max_iter, min_iter, threads, base):
    w, h, box, ship = CANVASES[canvas]
    hist, cnt, kernel, states = gpu_launches(cb, w, h, box, max_iter, min_iter, threads, [100], base, ship)
    assert kernel == (LOCKSTEP if base else PRODUCT)
    st = oracle.init_states(1337, 0, threads)
    want, wc = oracle.render(w, h, max_iter, min_iter, threads, 2, box=box, states=st, burning_ship=ship,
                             omp_threads=omp_threads())
    assert cnt["status"] == 0
    assert {k: cnt[k] for k in wc} == wc, (cnt, wc)
    assert np.array_equal(hist, want)
    assert np.array_equal(states, planar_states(st))
    assert int(hist.sum()) == cnt["increments"] > 0
    if base:
        assert cnt["skipped_steps"] == 0
    elif max_iter >= 1000 and not ship:
        assert cnt["skipped_steps"] > 0  # the early-out retired orbits


def test_focus_launches_refuse_what_they_do_not_define(cb):
    import torch

    dims = cb.FractalDimensions.make(64, 64)
    it = cb.IterationControl(100, 20)
    bufs = Launches(cb, dims, 64, planes=16)  # 1 << 16 words
    buf, states = bufs.out, bufs.states
    torch.cuda.synchronize()
    draw = cb.lib.cb_draw_buddhabrot_focus
    args = (C.byref(dims), buf.data_ptr(), C.byref(it), states.data_ptr(), 64, 1, None)
    assert draw(*args, cb.CB_KERNEL_DEFAULT, 6, buf.data_ptr(), 0, None) == 1       # n_cells = 0
    assert draw(*args, cb.CB_KERNEL_DEFAULT, 6, None, 5, None) == 1                 # no list
    assert draw(*args, cb.CB_KERNEL_DEFAULT, 3, buf.data_ptr(), 5, None) == 1       # level out of range
    assert draw(*args, cb.CB_KERNEL_DEFAULT, 11, buf.data_ptr(), 5, None) == 1
    assert draw(*args, cb.CB_KERNEL_DEFAULT, 0, buf.data_ptr(), 5, None) == 1
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN):
        assert draw(*args, variant, 0, None, 0, None) == 1
        assert cb.lib.cb_focus_probe(C.byref(dims), C.byref(it), states.data_ptr(), 64, 1, 6, buf.data_ptr(), None,
                                     variant, None) == 1
    assert cb.lib.cb_focus_probe(C.byref(dims), C.byref(it), states.data_ptr(), 64, 1, 3, buf.data_ptr(), None, 0,
                                 None) == 1
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ---- 2. the probe ---------------------------------------------------------------------------------------------------

PROBES = [(name, level, m, c) for name in focus.BOXES for level in (5, 8) for m, c in ((500, 20), (2000, 200))]


@pytest.fixture(scope="module")
def probed(ref):
    """The restatement's probe of every case, once: (mask, counters)."""
    out = {}
    for name, level, m, c in PROBES:
        out[name, level, m, c] = focus.probe(ref, 256, 256, m, c, 4096, PROBE_LAUNCHES, level, focus.BOXES[name],
                                             omp_threads=omp_threads())
    return out


@pytest.mark.parametrize("name,level,m,c", PROBES)
def test_probe_equals_the_restatement(cb, probed, name, level, m, c):
    want, wc = probed[name, level, m, c]
    bits = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 0 < bits < (4 << level) ** 2  # the case marks a cell and leaves one unmarked, or it tests nothing
    assert wc["recorded"] >= bits and wc["increments"] == 0
    states = None
    for base, kernel_id in ((cb.CB_KERNEL_SIMPLE, LOCKSTEP), (cb.CB_KERNEL_DEFAULT, PRODUCT)):
        mask, cnt, kernel, st = gpu_launches(cb, 256, 256, focus.BOXES[name], m, c, 4096, PROBE_LAUNCHES, base,
                                             level=level, probe=True)
        assert kernel == kernel_id
        assert_same((mask, cnt), (want, wc))
        assert states is None or np.array_equal(states, st)
        states = st


def test_probe_of_the_burning_ship_equals_the_restatement(cb, ref):
    box = (-1.8, -1.7, -0.1, 0.0)  # the ship's bow
    want, wc = focus.probe(ref, 128, 128, 300, 10, 4000, [50, 137], 6, box, ship=True, omp_threads=omp_threads())
    assert 0 < int(np.unpackbits(want.view(np.uint8)).sum()) < 256 * 256
    for base in (cb.CB_KERNEL_SIMPLE, cb.CB_KERNEL_DEFAULT):
        mask, cnt, _, _ = gpu_launches(cb, 128, 128, box, 300, 10, 4000, [50, 137], base, ship=True, level=6, probe=True)
        assert_same((mask, cnt), (want, wc))


# ---- 3. the focused draw ----------------------------------------------------------------------------------------------


def check_focused_draw(cb, ref, w, h, box, m, c, threads, launches, level, cells, ship=False):
    want, wc = focus.draw(ref, w, h, m, c, threads, launches, box=box, level=level, cell_list=cells, ship=ship,
                          omp_threads=omp_threads())
    l_hist, l_cnt, l_kernel, l_states = gpu_launches(cb, w, h, box, m, c, threads, launches, cb.CB_KERNEL_SIMPLE, ship,
                                                     level, cells)
    p_hist, p_cnt, p_kernel, p_states = gpu_launches(cb, w, h, box, m, c, threads, launches, cb.CB_KERNEL_DEFAULT, ship,
                                                     level, cells)
    assert (l_kernel, p_kernel) == (LOCKSTEP, PRODUCT)
    assert l_cnt["skipped_steps"] == 0
    assert_same((l_hist, l_cnt), (want, wc))
    assert_same((p_hist, p_cnt), (l_hist, l_cnt))
    assert np.array_equal(p_states, l_states)
    assert wc["samples"] == threads * sum(launches) and int(want.sum()) == wc["increments"]
    return wc, p_cnt


@pytest.mark.parametrize("name,level,m,c", PROBES)
def test_focused_draw_on_probed_lists(cb, ref, probed, name, level, m, c):
    cells = focus.cells(ref, level, probed[name, level, m, c][0], 1)
    wc, _ = check_focused_draw(cb, ref, 256, 256, focus.BOXES[name], m, c, 4096, [1, 50, 137], level, cells)
    assert wc["increments"] > 0


def planted_lists(level):
    n = 4 << level
    valley = (17 * n // 32) * n + 5 * n // 16  # the cell with the corner -0.75 + 0.125i: above the seahorse valley
    return {
        "one": np.array([valley], dtype=np.uint32),
        "all": np.arange(n * n, dtype=np.uint32),
        "edges": np.array([n // 2, n * (n // 2), n * (n // 2) + n - 1, n * (n - 1) + n // 2, 0, n * n - 1, valley],
                          dtype=np.uint32),
    }


@pytest.mark.parametrize("kind", ["one", "all", "edges"])
@pytest.mark.parametrize("level", [4, 10])
def test_focused_draw_on_planted_lists(cb, ref, level, kind):
    cells = planted_lists(level)[kind]
    wc, _ = check_focused_draw(cb, ref, 256, 256, SQUARE, 500, 20, 4000, [1, 50, 137], level, cells)
    assert wc["increments"] > 0 and wc["recorded"] > 0


@pytest.mark.parametrize("max_iter", [60, 119, 120, 121, 180, 1000])
@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "burning_ship"])
def test_focused_draw_at_chunk_boundaries(cb, ref, probed, max_iter, ship):
    """Cells along the set's boundary hold the orbits that never escape and fall into exact cycles; a point is first
    saved at 60 and first matched at 120, so the early-out decides at, one before and one after a chunk boundary."""
    if ship:
        level, box = 6, (-1.8, -1.7, -0.1, 0.0)
        mask, _ = focus.probe(ref, 128, 128, 300, 10, 4096, [50] * 4, level, box, ship=True, omp_threads=omp_threads())
        w = h = 128
    else:
        level, box, w, h = 5, focus.BOXES["body"], 256, 256
        mask = probed["body", 5, 500, 20][0]
    cells = focus.cells(ref, level, mask, 1)
    assert 0 < cells.size < (4 << level) ** 2
    wc, p_cnt = check_focused_draw(cb, ref, w, h, box, max_iter, 10, 4096, [50, 50], level, cells, ship)
    assert wc["never_escaped"] > 0
    print("max_iter %d: %d of %d iterate steps skipped" % (max_iter, p_cnt["skipped_steps"], p_cnt["iterate_steps"]))
    if max_iter <= 120:  # a match at 120 == max_iter skips nothing
        assert p_cnt["skipped_steps"] == 0
    if max_iter == 1000:  # tens of thousands of orbits inside the bulbs: some are exact cycles long before 1000
        assert p_cnt["skipped_steps"] > 0


# ---- 4. renderer and CLI ----------------------------------------------------------------------------------------------


def restated_render(ref, w, h, box, m, c, threads, probe_passes, passes, level=8, dilate=1, ship=False):
    """What cb_renderer_set_focus + render_passes define: the probe on fresh generators, the list, the focused passes on
    fresh generators of the same subsequences -> (hist, counters, cells)."""
    mask, _ = focus.probe(ref, w, h, m, c, threads, [50] * probe_passes, level, box, ship=ship, omp_threads=omp_threads())
    cells = focus.cells(ref, level, mask, dilate)
    hist, cnt = focus.draw(ref, w, h, m, c, threads, [50 * passes], box=box, level=level, cell_list=cells, ship=ship,
                           omp_threads=omp_threads())
    return hist, cnt, cells


@pytest.mark.parametrize("base", [0, 1], ids=["product", "lockstep"])
def test_renderer_set_focus_and_three_passes(cb, ref, base):
    w = h = 256
    box, m, c, threads = focus.BOXES["body"], 500, 20, 4096
    want, wc, cells = restated_render(ref, w, h, box, m, c, threads, 8, 3, level=6)
    dims = cb.FractalDimensions.make(w, h, *box)
    with cb.Renderer(dims, cb.IterationControl(m, c), device=0, n_threads=threads) as r:
        assert r.focus_cells() == (0, 0)
        assert r.set_focus(6, 8, 1, base) == (cells.size, 256 * 256)
        before = r.read_rng_states().copy()
        r.render_passes(1, base)
        r.render_passes(2, base)
        assert cb.lib.cb_debug_last_draw_kernel() == (LOCKSTEP if base else PRODUCT)
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
        # once focused: no second focus, no anti passes, no other step
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 8, 1, base) == 1
        assert cb.lib.cb_renderer_render_passes(r._h, 1, base | cb.CB_KERNEL_FLAG_ANTI) == 1
        assert cb.lib.cb_renderer_render_passes(r._h, 1, base | cb.CB_KERNEL_FLAG_BURNING_SHIP) == 1
    assert_same((hist, cnt), (want, wc))
    with cb.Renderer(dims, cb.IterationControl(m, c), device=0, n_threads=threads) as fresh:
        assert np.array_equal(before, fresh.read_rng_states())  # the probe ran on generators of its own


def test_renderer_refuses_focus_where_it_is_not_defined(cb):
    dims = cb.FractalDimensions.make(64, 64, *focus.BOXES["body"])
    with cb.Renderer(dims, [(100, 20), (50, 5)], device=0, n_threads=1024) as r:
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == 1  # a channel renderer
    with cb.Renderer(dims, cb.IterationControl(100, 20), device=0, n_threads=1024) as r:
        for level, probe, dilate, variant in ((3, 2, 1, 0), (11, 2, 1, 0), (6, 0, 1, 0), (6, 2, -1, 0),
                                              (6, 2, 1, cb.CB_KERNEL_FLAG_ANTI), (6, 2, 1, cb.CB_KERNEL_TIMED)):
            assert cb.lib.cb_renderer_set_focus(r._h, level, probe, dilate, variant) == 1
        r.render_passes(1)
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == 1  # after the first pass
    far = cb.FractalDimensions.make(64, 64, 10.0, 10.05, 10.0, 10.05)  # |z| <= 2^2 + |c| < 7: no orbit comes here
    with cb.Renderer(far, cb.IterationControl(100, 20), device=0, n_threads=1024) as r:
        assert cb.lib.cb_renderer_set_focus(r._h, 6, 2, 1, 0) == cb.CB_ERROR_FOCUS_EMPTY
        assert r.focus_cells() == (0, 0)
        with pytest.raises(cb.CudabrotError) as e:
            r.set_focus(6, 2, 1)
        assert e.value.code == cb.CB_ERROR_FOCUS_EMPTY and "probe" in str(e.value)


def box_flags(box):
    return ["--min-real", repr(box[0]), "--max-real", repr(box[1]), "--min-imag", repr(box[2]), "--max-imag", repr(box[3])]


@pytest.mark.parametrize("extra", [[], ["--kernel", "simple"]], ids=["product", "lockstep"])
def test_cli_focus_image_equals_the_restatement(exe, ref, cb, oracle, tmp_path, extra):
    box = focus.BOXES["body"]
    out = str(tmp_path / "focus.pgm")
    r = run(exe, "--focus-level", "6", "--focus-probe", "2", "-w", "128", "-h", "128", "-m", "300", "-c", "20",
            "--passes", "2", "--stats", "-o", out, *box_flags(box), *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    want, wc, cells = restated_render(ref, 128, 128, box, 300, 20, 512 * 512, 2, 2, level=6)
    assert "Focus: sampling %d of 65536 cells of side 2^-6 (2 probe passes, dilated by 1)." % cells.size in r.stdout
    assert '"focus_cells": %d, "focus_total": 65536' % cells.size in r.stderr
    assert '"increments": %d,' % wc["increments"] in r.stderr and '"samples": %d,' % wc["samples"] in r.stderr
    gray, _, _ = cb.set_grayscale_pixels(want, 1.0)
    with open(out, "rb") as f:
        assert f.read() == oracle.encode_pgm(gray)


def test_cli_focus_true_resume(exe, tmp_path):
    box = focus.BOXES["elephant"]
    common = ["--focus", "--focus-level", "5", "--focus-probe", "2", "-w", "200", "-h", "100", "-m", "200", "-o",
              os.devnull, *box_flags(box)]
    buf, side = str(tmp_path / "a.bin"), str(tmp_path / "a.rng")
    assert run(exe, "--passes", "2", "-s", buf, "--rng-state", side, *common).returncode == 0
    r2 = run(exe, "--passes", "1", "-s", buf, "--rng-state", side, *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    one_buf, one_side = str(tmp_path / "b.bin"), str(tmp_path / "b.rng")
    assert run(exe, "--passes", "3", "-s", one_buf, "--rng-state", one_side, *common).returncode == 0
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        whole = b.read()
        assert a.read() == whole and any(whole[32:])
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()


def test_cli_focus_with_an_empty_list_exits_1_without_an_image(exe, tmp_path):
    out = str(tmp_path / "none.pgm")
    r = run(exe, "--focus", "--focus-probe", "1", "-w", "64", "-h", "64", "--passes", "1", "-o", out, "--max-real",
            "10.05", "--min-real", "10", "--max-imag", "10.05", "--min-imag", "10")  # |z| <= 2^2 + |c| < 7
    assert r.returncode == 1
    assert "Focus: no sample of the 1 probe passes reaches the canvas; nothing to render." in r.stdout.split("\n")
    assert "Saving image." not in r.stdout and not os.path.exists(out)


# ---- 5. what the feature is for ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(focus.BOXES))
def test_focused_samples_reach_the_canvas_more_often(cb, ref, probed, name):
    """In-canvas increments per sample, focused against normal, same box and sample count, from the deterministic
    counters: the restatement computes both, the GPU must equal them, the focused ratio must be the larger one."""
    box, level, m, c, threads, launches = focus.BOXES[name], 8, 500, 20, 4096, [100]
    cells = focus.cells(ref, level, probed[name, level, m, c][0], 1)
    _, fc = focus.draw(ref, 256, 256, m, c, threads, launches, box=box, level=level, cell_list=cells,
                       omp_threads=omp_threads())
    _, nc = focus.draw(ref, 256, 256, m, c, threads, launches, box=box, omp_threads=omp_threads())
    _, g_fc, _, _ = gpu_launches(cb, 256, 256, box, m, c, threads, launches, cb.CB_KERNEL_DEFAULT, level=level,
                                 cell_list=cells)
    _, g_nc, _, _ = gpu_launches(cb, 256, 256, box, m, c, threads, launches, cb.CB_KERNEL_DEFAULT)
    assert_same((None, g_fc), (None, fc))
    assert_same((None, g_nc), (None, nc))
    focused, normal = fc["increments"] / fc["samples"], nc["increments"] / nc["samples"]
    n2 = (4 << level) ** 2
    print("%s: %d of %d cells (plane / list = %.1f); increments per sample focused %.5f, normal %.5f: %.1f x"
          % (name, cells.size, n2, n2 / cells.size, focused, normal, focused / normal if normal else float("inf")))
    assert focused > normal
