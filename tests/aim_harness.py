"""What the aimed render's GPU suites share (test_gpu_aim.py, test_gpu_aim_edges.py, test_gpu_aim_fuzz.py) -- test
infrastructure only: the fixture for the restatement (tests/aim_reference.c), the launches on the GPU through cb_aim_probe
and cb_draw_buddhabrot_aimed on device_launches' buffers, and the three-way comparison product kernels (30) == lock-step
kernel (31) == restatement on mask, list, histogram, generator states and counters.  A fixture imported into a test module
is a fixture of that module."""

import numpy as np
import pytest

import aim_reference as aim
import plot_reference as plot
from plot_harness import SAME, Launches, omp_threads, planar_states, variant_of, write_states

PRODUCT, LOCKSTEP = 30, 31
BASES = ((0, PRODUCT), (1, LOCKSTEP))  # (lock-step?, cb_debug_last_draw_kernel)


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return aim.load(tmp_path_factory.mktemp("aim_ref"))


def variant(cb, lockstep, s):
    return variant_of(cb, cb.CB_KERNEL_SIMPLE if lockstep else cb.CB_KERNEL_DEFAULT, s["degree"], s["ship"],
                      plot.code_of(s["formula"]))


def source_args(cb, s):
    return dict(iterations=cb.IterationControl(s["max_iter"], s["min_iter"]), projection=s["projection"], julia_c=s["c"],
                bounded=s["bounded"])


def gpu_probe(cb, lockstep, states=None, guard=0, **kw):
    """shape_of(kw)["probe"] launches of cb_aim_probe on fresh generators, or on the given oracle `states` written over them
    (they are left as they were), ORed into one mask -> (mask u32 words, counters, kernel, states).  guard: that many
    words allocated before and after the mask, and read back with it."""
    s = aim.shape_of(kw)
    bufs = Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"],
                    words=aim.mask_words(s["level"]) + 2 * guard, seed=s.get("seed"))
    if states is not None:
        write_states(bufs, states)

    def entry(d_hist, **args):  # the scaffolding's output buffer is the mask
        cb.aim_probe(d_mask=d_hist + 4 * guard, **args)

    return bufs.launches(entry, s["probe"], variant(cb, lockstep, s), level=s["level"], **source_args(cb, s)).read()


def gpu_draw(cb, lockstep, cell_list, states=None, **kw):
    """shape_of(kw)["draw"] launches of cb_draw_buddhabrot_aimed on fresh generators, or on the given oracle `states` written
    over them (they are left as they were), from `cell_list` (None: level 0, no cells, the uniform source) -> (hist [h, w],
    counters, kernel, states)."""
    s = aim.shape_of(kw)
    tables = {} if cell_list is None else {"cells": cell_list}
    bufs = Launches(cb, cb.FractalDimensions.make(s["w"], s["h"], *s["box"]), s["threads"], tables=tables, seed=s.get("seed"))
    if states is not None:
        write_states(bufs, states)
    grid = dict(level=0) if cell_list is None else dict(level=s["level"], d_cells=bufs.tables["cells"].data_ptr(),
                                                        n_cells=len(cell_list))
    return bufs.launches(cb.draw_buddhabrot_aimed, s["draw"], variant(cb, lockstep, s), **grid, **source_args(cb, s)).read()


def bits(mask):
    return int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())


def same_counters(cnt, want, what):
    assert cnt["status"] == 0, (what, cnt)
    assert {k: cnt[k] for k in SAME} == {k: want[k] for k in SAME}, (what, cnt, want)


def three_ways(cb, aref, oracle, **kw):
    """Probe, list and draw, each product == lock-step == restatement (naive and compressed) bit for bit -> dict(mask,
    cells, hist, probe=(counters, extra), draw=(counters, extra), product=the product draw's counters)."""
    s = aim.shape_of(kw)
    n_omp = omp_threads()
    # ---- the probe
    st = oracle.init_states(s.get("seed", 1337), 0, s["threads"])
    pex = {}
    mask, pc = aim.probe(aref, omp_threads=n_omp, states=st, extra=pex, **kw)
    probe_states = planar_states(st)
    mask1, pc1 = aim.probe(aref, mode=aim.COMPRESSED, omp_threads=n_omp, **kw)
    assert np.array_equal(mask1, mask) and {k: pc1[k] for k in SAME} == {k: pc[k] for k in SAME}
    assert pc["increments"] == 0 and pc["recorded"] == pex["marking"]
    for lockstep, kernel in BASES:
        got, cnt, launched, after = gpu_probe(cb, lockstep, **kw)
        print("probe", kernel, cnt)
        assert launched == kernel
        same_counters(cnt, pc, ("probe", kernel))
        assert np.array_equal(got, mask), ("probe", kernel)
        assert np.array_equal(after, probe_states), ("probe", kernel)
    # ---- the list: the library's host function against the restatement's
    cells = aim.cells(aref, mask, **kw)
    assert np.array_equal(cb.focus_cells(s["level"], mask, s["dilate"]), cells)
    out = dict(mask=mask, cells=cells, probe=(pc, pex))
    if len(cells) == 0:
        return out
    # ---- the draw
    st = oracle.init_states(s.get("seed", 1337), 0, s["threads"])
    dex = {}
    want, dc = aim.draw(aref, cells, omp_threads=n_omp, states=st, extra=dex, **kw)
    draw_states = planar_states(st)
    want1, dc1 = aim.draw(aref, cells, mode=aim.COMPRESSED, omp_threads=n_omp, **kw)
    assert np.array_equal(want1, want) and {k: dc1[k] for k in SAME} == {k: dc[k] for k in SAME}
    assert dc["samples"] == s["threads"] * sum(s["draw"]) and int(want.sum()) == dc["increments"]
    for lockstep, kernel in BASES:
        hist, cnt, launched, after = gpu_draw(cb, lockstep, cells, **kw)
        print("draw", kernel, cnt)
        assert launched == kernel
        same_counters(cnt, dc, ("draw", kernel))
        assert np.array_equal(hist, want), ("draw", kernel)
        assert np.array_equal(after, draw_states), ("draw", kernel)
        if lockstep:
            assert cnt["skipped_steps"] == 0
        else:
            out["product"] = cnt
            if s["bounded"]:  # the bounded suites' rule: the compressed restatement's discount
                assert cnt["skipped_steps"] == dc1["skipped_steps"], (cnt, dc1)
    out.update(hist=want, draw=(dc, dex))
    return out
