"""The aimed render's CPU restatement (tests/aim_reference.c) against itself and against the restatements it is built
beside, and the public surface, without a GPU:

  1. a bounded orbit replayed naively and cycle-compressed gives the same probe (mask, replay_steps and every other counter)
     and the same draw, for all 13 steps and both sources of c;
  2. the draw with no list is tests/plot_reference.c's projected render and tests/bounded_reference.c's bounded one;
  3. with the identity matrix, the reference's step, a sampled c and escaping orbits, probe, list and draw are
     tests/focus_reference.c's: mask, list, histogram, generator states and counters; and the six-draw mapping is its own;
  4. the issue's table: every case reaches what the model says it reaches;
  5. the header, the Python names and the error text.
"""

import os

import numpy as np
import pytest

import aim_reference as aim
import bounded_reference as bounded
import focus_reference as focus
import plot_reference as plot
from device_launches import SAME, omp_threads, planar_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = ([dict(), dict(ship=True)] + [dict(degree=d) for d in range(3, 9)]
         + [dict(formula=f) for f in ("tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn")])
STEP_IDS = ["reference", "ship"] + ["power%d" % d for d in range(3, 9)] + ["tricorn", "celtic", "buffalo", "perpendicular",
                                                                          "celtic-tricorn"]
# small on purpose: 200 threads, M = 500 (eight chunk boundaries), a crop of the (z_re, c_re) plane or of a Julia set's z
SMALL = dict(threads=200, probe=(2, 6), draw=(2, 9, 1))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return aim.load(tmp_path_factory.mktemp("aim_ref"))


def popcount(mask):
    return int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())


@pytest.mark.parametrize("source", ["sampled", "fixed"])
@pytest.mark.parametrize("step", STEPS, ids=STEP_IDS)
def test_naive_equals_compressed_for_the_bounded_probe_and_draw(aref, step, source):
    kw = dict(SMALL, bounded=True, **step)
    if source == "fixed":
        kw.update(c=(0.1, 0.1), box=(-0.4, 0.4, -0.4, 0.4))  # a c whose Julia set has an interior under every step
    else:
        kw.update(projection=aim.ZR_CR, box=(-0.6, 0.6, -0.75, 0.25))
    ex = {}
    mask, pc = aim.probe(aref, extra=ex, **kw)
    mask1, pc1 = aim.probe(aref, mode=aim.COMPRESSED, **kw)
    assert np.array_equal(mask, mask1)
    assert {k: pc[k] for k in SAME} == {k: pc1[k] for k in SAME}  # replay_steps: the first in-canvas index is the naive one
    assert pc["recorded"] == ex["marking"] >= popcount(mask) > 0 and pc["increments"] == 0
    cells = aim.cells(aref, mask, **kw)
    dex = {}
    hist, dc = aim.draw(aref, cells, extra=dex, **kw)
    hist1, dc1 = aim.draw(aref, cells, mode=aim.COMPRESSED, **kw)
    assert np.array_equal(hist, hist1) and {k: dc[k] for k in SAME} == {k: dc1[k] for k in SAME}
    assert dc["skipped_steps"] == 0 and int(hist.sum()) == dc["increments"] == dex["in_canvas"] > 0
    assert dc["replay_steps"] == 500 * dc["recorded"] == dex["in_canvas"] + dex["off_canvas"]
    assert dex["cycles"] > 0  # the compressed path is taken
    assert dc1["skipped_steps"] > 0


@pytest.mark.parametrize("kw", [
    dict(), dict(ship=True), dict(degree=3, projection=aim.ZR_CR), dict(formula="tricorn", c=(0.1, 0.1), min_iter=2),
    dict(c=(-0.123, 0.745), box=(0.2, 0.7, 0.2, 0.7)), dict(projection=aim.ZR_CR, box=(-1.0, -0.5, -1.5, -1.25)),
], ids=["identity", "ship", "power3", "tricorn_julia", "julia_crop", "zr_cr_crop"])
def test_the_draw_with_no_list_is_the_projected_render(aref, kw):
    s = aim.shape_of(dict(SMALL, **kw))
    pref = plot.load(os.path.dirname(aref._name))
    st0, st1 = aim_states(s), aim_states(s)
    got, gc = aim.draw(aref, None, states=st0, **dict(SMALL, **kw))
    want, wc = plot.draw(pref, s["w"], s["h"], s["max_iter"], s["min_iter"], s["threads"], list(s["draw"]),
                         projection=s["projection"], degree=s["degree"], ship=s["ship"], formula=s["formula"], c=s["c"],
                         box=s["box"], states=st1)
    assert np.array_equal(got, want) and {k: gc[k] for k in SAME} == {k: wc[k] for k in SAME}
    assert np.array_equal(planar_states(st0), planar_states(st1))
    assert gc["recorded"] > 0 and (gc["rejected"] > 0) == aim.rejects(s)


def aim_states(s):
    from oracle import binding

    return binding.init_states(1337, 0, s["threads"])


@pytest.mark.parametrize("kw", [
    dict(), dict(ship=True, projection=aim.ZR_CR), dict(degree=4), dict(formula="celtic", c=(-0.4, 0.3)),
    dict(c=(-1.0, 0.0), box=(-0.5, 0.5, -0.5, 0.5)), dict(projection=aim.ZR_CR, box=(-2.0, 2.0, -1.5, -1.25)),
], ids=["identity", "ship", "power4", "celtic_julia", "julia_crop", "zr_cr_crop"])
@pytest.mark.parametrize("mode", [aim.NAIVE, aim.COMPRESSED], ids=["naive", "compressed"])
def test_the_draw_with_no_list_is_the_bounded_render(aref, kw, mode):
    s = aim.shape_of(dict(SMALL, bounded=True, **kw))
    bref = bounded.load(os.path.dirname(aref._name))
    st0, st1 = aim_states(s), aim_states(s)
    got, gc = aim.draw(aref, None, mode=mode, states=st0, **dict(SMALL, bounded=True, **kw))
    want, wc = bounded.draw(bref, s["w"], s["h"], s["max_iter"], s["threads"], list(s["draw"]), projection=s["projection"],
                            degree=s["degree"], ship=s["ship"], formula=s["formula"], c=s["c"], box=s["box"], mode=mode,
                            states=st1)
    assert np.array_equal(got, want) and gc == wc  # skipped_steps too
    assert np.array_equal(planar_states(st0), planar_states(st1))
    assert gc["recorded"] > 0 and gc["rejected"] == 0


@pytest.mark.parametrize("ship,box", [(False, focus.BOXES["body"]), (False, focus.BOXES["elephant"]),
                                      (True, (-1.8, -1.7, -0.1, 0.0))], ids=["body", "elephant", "ship"])
def test_the_identity_case_is_the_focused_render(aref, ship, box):
    kw = dict(box=box, ship=ship)
    s = aim.shape_of(kw)
    fref = aref.focus
    st0, st1 = aim_states(s), aim_states(s)
    mask, pc = aim.probe(aref, states=st0, **kw)
    fmask, fpc = focus.probe(fref, s["w"], s["h"], s["max_iter"], s["min_iter"], s["threads"], list(s["probe"]), s["level"], box,
                             ship=ship, states=st1)
    assert np.array_equal(mask, fmask) and {k: pc[k] for k in SAME} == fpc and popcount(mask) > 0
    assert np.array_equal(planar_states(st0), planar_states(st1))
    cells = aim.cells(aref, mask, **kw)
    assert 0 < len(cells) < (4 << s["level"]) ** 2
    st0, st1 = aim_states(s), aim_states(s)
    hist, dc = aim.draw(aref, cells, states=st0, **kw)
    fhist, fdc = focus.draw(fref, s["w"], s["h"], s["max_iter"], s["min_iter"], s["threads"], list(s["draw"]), box=box,
                            level=s["level"], cell_list=cells, ship=ship, states=st1)
    assert np.array_equal(hist, fhist) and {k: dc[k] for k in SAME} == fdc and dc["increments"] > 0
    assert np.array_equal(planar_states(st0), planar_states(st1))


def test_the_six_draw_mapping_is_the_focused_renders(aref):
    rng = np.random.default_rng(23)
    for level in (4, 6, 10):
        n = 4 << level
        cells = np.unique(rng.integers(0, n * n, 37, dtype=np.uint32))
        edge = [0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff]
        for trial in range(200):
            draws = [int(rng.choice(edge)) if rng.random() < 0.3 else int(rng.integers(0, 1 << 32)) for _ in range(6)]
            assert aim.mapping(aref, level, cells, *draws) == focus.mapping(aref.focus, level, cells, *draws)


def test_the_library_lists_cells_as_the_restatement_does(aref, cb):
    """cb_focus_mask_bytes and cb_focus_cells serve the aimed render unchanged (host arithmetic: no device)."""
    kw = aim.CASES["bounded_zr_cr"]
    s = aim.shape_of(kw)
    mask, _ = aim.probe(aref, omp_threads=omp_threads(), **kw)
    assert cb.focus_mask_bytes(s["level"]) == 4 * mask.size
    for dilate in (0, 1, 2):
        assert np.array_equal(cb.focus_cells(s["level"], mask, dilate), aim.cells(aref, mask, **dict(kw, dilate=dilate)))


# ---- 4. the issue's table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(aim.CASES))
def test_every_case_of_the_table_reaches_its_paths(aref, name):
    case = aim.CASES[name]
    s = aim.shape_of(case)
    pex, dex = {}, {}
    mask, pc = aim.probe(aref, omp_threads=omp_threads(), extra=pex, **case)
    cells = aim.cells(aref, mask, **case)
    hist, dc = aim.draw(aref, cells, mode=aim.COMPRESSED, omp_threads=omp_threads(), extra=dex, **case)
    print(name, "probe", pc, pex, "draw", dc, dex)
    assert (popcount(mask), len(cells)) == (case["marked"], case["listed"])
    assert 0 < len(cells) < (4 << s["level"]) ** 2
    assert dex["in_canvas"] > 0 and dex["off_canvas"] > 0  # every window is a crop
    if "plotted" in case:
        assert dex["plotted"] == dc["recorded"] == case["plotted"]
    if "cycles" in case:
        assert (dex["cycles"], dex["no_cycle"]) == (case["cycles"], case["no_cycle"])
    if s["bounded"]:
        assert dex["both_weights"] > 0 and dc["rejected"] == 0
        if s["c"] is None:
            assert dex["cycles"] > 0 and dex["no_cycle"] > 0  # both cycle outcomes with a sampled c
    else:
        assert dc["never_escaped"] > 0  # never-escaping samples among the escaping kind's
        assert (dc["rejected"] > 0) == aim.rejects(s)
    if name == "plane_zr_cr":
        assert (dc["recorded"], dc["never_escaped"], dc["rejected"]) == (22437, 5720, 1096)
    if name == "bounded_julia":
        assert dex["cycles"] == 48506 == dex["both_weights"] and dex["no_cycle"] == 0


def test_a_probe_that_marks_nothing(aref):
    kw = dict(aim.CASES["bounded_zr_cr"], box=(-2.0, 2.0, -1.79, -1.74))
    mask, pc = aim.probe(aref, omp_threads=omp_threads(), **{k: v for k, v in kw.items() if k not in aim.MODEL_KEYS})
    assert not mask.any() and pc["recorded"] == 0 and pc["never_escaped"] > 0
    assert pc["replay_steps"] == 500 * pc["never_escaped"]  # every bounded orbit replayed to its end, off the canvas


# ---- 5. the public surface ----------------------------------------------------------------------------------------------


def test_the_header_declares_the_aimed_render():
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert "#define CB_ERROR_AIM_EMPTY 100003" in text
    assert "/* ---- Aimed render:" in text
    for name in ("cb_aim_probe", "cb_draw_buddhabrot_aimed", "cb_renderer_set_aim", "cb_renderer_aim_cells"):
        assert "int %s(" % name in text, name
    assert "30 the\n * aim product kernels" in text and "31 the aim lock-step kernel" in text


def test_the_package_exports_the_aimed_render(cb):
    for name in ("aim_probe", "draw_buddhabrot_aimed", "CB_ERROR_AIM_EMPTY", "Renderer"):
        assert name in cb.__all__ and hasattr(cb, name), name
    assert cb.CB_ERROR_AIM_EMPTY == 100003 != cb.CB_ERROR_FOCUS_EMPTY
    assert callable(cb.Renderer.set_aim) and callable(cb.Renderer.aim_cells)
    for symbol in ("cb_aim_probe", "cb_draw_buddhabrot_aimed", "cb_renderer_set_aim", "cb_renderer_aim_cells"):
        assert hasattr(cb.lib, symbol), symbol
    text = cb.lib.cb_error_string(cb.CB_ERROR_AIM_EMPTY)
    text = text.decode() if isinstance(text, bytes) else text
    assert "aim probe marked no cell" in text


def test_entry_points_refuse_null_arguments_without_a_device(cb):
    """What is refused before anything touches a device: hipErrorInvalidValue (1)."""
    import ctypes as C

    dims, it = cb.FractalDimensions.make(16, 16), cb.IterationControl(100, 20)
    p = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    assert cb.lib.cb_aim_probe(C.byref(dims), C.byref(it), p, None, 0, None, 64, 1, 6, None, None, 0, None) == 1
    assert cb.lib.cb_draw_buddhabrot_aimed(C.byref(dims), None, C.byref(it), p, None, 0, None, 64, 1, None, 0, 0, None, 0,
                                           None) == 1
    assert cb.lib.cb_renderer_set_aim(None, 6, 4, 1, 0) == 1
    assert cb.lib.cb_renderer_aim_cells(None, None, None) == 1
