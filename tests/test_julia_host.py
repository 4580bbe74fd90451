"""The Julia render (include/cudabrot_amd.h, "Julia render") without a GPU, and with it every setting of the plotted
renders' one CPU restatement (tests/plot_reference.c): pinned to a pure-Python restatement of the definitions on the
oracle's generator -- a fixed and a sampled c, with and without rejection, a table, every formula, a depth with and
without its table --, its step pinned to
z^d + c in exact rational arithmetic, and its independence of the OpenMP thread count."""

import ctypes as C
import math
from fractions import Fraction as F

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import ref  # noqa: F401


# ---- 1. the C restatement is the definition ---------------------------------------------------------------------------


def fma(a, b, c):
    """One rounding: math.fma where Python has it, else the exact rational value rounded to nearest even (all operands
    here are finite)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(F(a) * F(b) + F(c))


def py_step(cr, ci, r, i, degree=2, ship=False, formula=0):
    """The step of the definition in Python's own IEEE doubles -> (r', i', |z'|^2): the header's table for a formula
    code, else the reference's step or its Burning Ship variant (degree 2), else the repeated product."""
    if formula or degree == 2:
        ii = i * i
        t = fma(r, r, -ii)
        real_part, a, b = {
            0: (t, abs(r) + abs(r), abs(i)) if ship else (t, r + r, i),
            1: (t, -(r + r), i),
            2: (abs(t), r + r, i),
            3: (abs(t), abs(r) + abs(r), abs(i)),
            4: (t, -(abs(r) + abs(r)), i),
            5: (abs(t), -(r + r), i),
        }[formula]
        nr = cr + real_part
        ni = fma(a, b, ci)
    else:
        wr, wi = r, i
        for _ in range(degree - 1):
            t = wi * i
            pr = fma(wr, r, -t)
            s = wi * r
            pi = fma(wr, i, s)
            wr, wi = pr, pi
        nr, ni = cr + wr, ci + wi
    return nr, ni, fma(ni, ni, nr * nr)


def py_draw(oracle, w, h, box, max_iter, min_iter, threads, samples, p, states, c=None, degree=2, ship=False, formula=0,
            lut=None, reject=False, depth=None, notes=None):
    """The definition, sample by sample, on the oracle's generator -> (hist, counters).  c None: c is the sample; reject:
    the oracle's two shortcuts drop the sample; lut: three planes of the entry's bytes; depth = (row, min, max, N): N
    planes, a point in the plane of its slice and none outside the window -- or, with lut, three planes of the bytes of
    the slice's entry.  A given dict `notes` receives the on-canvas points dropped for their depth and the slices hit."""
    d = oracle.make_dims(w, h, *box)
    row_d, lo, hi, slices = (None, 0.0, 0.0, 0) if depth is None else (plot.row_of(depth[0]),) + tuple(depth[1:])
    hist = np.zeros((3, h, w) if lut is not None else (h, w) if depth is None else (slices, h, w), dtype=np.uint64)
    planes = hist.reshape(-1, h, w)
    dropped, hit = 0, set()
    cnt = dict.fromkeys(plot.COUNTER_NAMES, 0)
    for t in range(threads):
        g = oracle.Xorwow.from_buffer(states, t * states.dtype.itemsize)
        for _ in range(samples):
            sr = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            si = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            cr, ci = (sr, si) if c is None else c
            cnt["samples"] += 1
            if reject and (oracle.lib.orc_in_main_cardioid(sr, si) or oracle.lib.orc_in_order2_bulb(sr, si)):
                cnt["rejected"] += 1
                continue
            r, i, k = sr, si, max_iter
            for n in range(max_iter):
                r, i, m = py_step(cr, ci, r, i, degree, ship, formula)
                if m > 4.0:
                    k = n
                    break
            if k >= max_iter:
                cnt["never_escaped"] += 1
                cnt["iterate_steps"] += max(max_iter, 0)
                continue
            cnt["iterate_steps"] += k + 1
            if k < min_iter:
                cnt["too_fast"] += 1
                continue
            cnt["recorded"] += 1
            entry = 1 if lut is None or depth is not None else int(lut[k])  # a table by escape index
            ku = fma(p[2], cr, p[3] * ci)
            kv = fma(p[6], cr, p[7] * ci)
            kd = 0.0 if depth is None else fma(row_d[2], cr, row_d[3] * ci)
            r, i = sr, si
            for _ in range(k + 1):
                r, i, _ = py_step(cr, ci, r, i, degree, ship, formula)
                cnt["replay_steps"] += 1
                u = fma(p[0], r, fma(p[1], i, ku))
                v = fma(p[4], r, fma(p[5], i, kv))
                if u < d.min_real or v < d.min_imag:
                    continue
                col, row = int((u - d.min_real) / d.delta_real), int((v - d.min_imag) / d.delta_imag)
                if not (0 <= col < w and 0 <= row < h):
                    continue
                first = 0
                if depth is not None:
                    dd = fma(row_d[0], r, fma(row_d[1], i, kd))
                    s = -1 if dd < lo else int((dd - lo) / ((hi - lo) / float(slices)))
                    if not 0 <= s < slices:
                        dropped += 1
                        continue
                    hit.add(s)
                    if lut is None:
                        first = s
                    else:
                        entry = int(lut[s]) & 0xFFFFFF  # a table by slice
                for j in range(3):
                    weight = (entry >> (8 * j)) & 255
                    if weight:
                        planes[first + j, row, col] += weight
                        cnt["increments"] += weight
    if notes is not None:
        notes.update(dropped_for_depth=dropped, slices=hit)
    return hist, cnt


# The settings of the one restatement, each at 64 x 64, 8 threads x 20 samples, -m 200 -c 2 (min_iter where it is not 2).
# A fixed c: degree 2, the ship, the smallest and the largest Multibrot degree; one on another plane, so that K_u and K_v
# from the fixed c are part of what is compared.  Then one case per other axis: the sampled c with the product's
# rejection and without any, a table on either source of c, each formula, and a formula with a fixed c and a table.  Each
# was checked with py_draw to record and plot something (to reject something, to fill two planes) before it was fixed.
# Then the two sinks of a depth: without a table on a sampled c with rejection and on a fixed c, with a table on a sampled
# c (an irrational row) and under a formula.  Their windows are cut inside the set, so that on-canvas points fall outside
# them, and every entry of their tables lacks a colour; the test asserts both, and that two slices are hit.
C_JULIA = (-0.8, 0.156)
SLICE_TABLE = np.array([0x0000FF, 0x00FF00, 0x030000, 0x000201, 0x7F0001, 0x00FF00], dtype=np.uint32)
TINY = {
    "z2": dict(c=C_JULIA),
    "z2_hologram": dict(c=C_JULIA, projection=plot.HOLOGRAM),
    "ship": dict(c=C_JULIA, ship=True),
    "d3": dict(c=(0.0, 0.0), degree=3),
    "d8": dict(c=(0.4, 0.2), degree=8, min_iter=0),
    "sampled_rejecting": dict(reject=True),
    "sampled_d3_not_rejecting": dict(degree=3, reject=False),
    "window_table_fixed_c": dict(c=C_JULIA, lut=plot.window_table(200, [(2, 6), (6, 200), (4, 12)])),
    "demo_table_sampled": dict(lut=plot.demo_table(200), reject=True),
    "tricorn": dict(formula=1),
    "celtic": dict(formula=2),
    "buffalo": dict(formula=3),
    "perpendicular": dict(formula=4),
    "celtic_tricorn": dict(formula=5),
    "tricorn_fixed_c_table": dict(formula=1, c=C_JULIA, lut=plot.demo_table(200), projection=plot.HOLOGRAM),
    "depth_sampled_rejecting": dict(depth=("cr", -1.5, 0.4, 5), reject=True),
    "depth_fixed_c": dict(c=C_JULIA, depth=("zi", -0.5, 0.6, 4)),
    "depth_table_sampled": dict(depth=(plot.HOLOGRAM[1], -0.7, 0.9, 6), lut=SLICE_TABLE, reject=True),
    "depth_table_tricorn": dict(formula=1, depth=("zr", -1.0, 0.5, 5), lut=SLICE_TABLE[:5]),
}


@pytest.mark.parametrize("case", list(TINY))
def test_c_restatement_is_the_python_restatement(ref, oracle, case):
    kw = dict(TINY[case])
    w = h = 64
    box = (-2.0, 2.0, -2.0, 2.0)
    max_iter, min_iter, threads, samples = 200, kw.pop("min_iter", 2), 8, 20
    p = kw.pop("projection", plot.IDENTITY)
    reject = kw.pop("reject", False)
    own = oracle.init_states(1337, 0, threads)
    notes = {}
    want, wc = py_draw(oracle, w, h, box, max_iter, min_iter, threads, samples, plot.matrix(p), own, reject=reject,
                       notes=notes, **kw)
    states = oracle.init_states(1337, 0, threads)
    # reject=True is what the product's rule (reject=None) gives in those cases: that rule is part of what is compared
    hist, cnt = plot.draw(ref, w, h, max_iter, min_iter, threads, [samples], projection=p, box=box, states=states,
                          reject=None if reject else False, **kw)
    assert wc["samples"] == threads * samples and (wc["rejected"] > 0) == reject
    assert wc["recorded"] > 0 and wc["increments"] > 0
    assert wc["rejected"] + wc["never_escaped"] + wc["too_fast"] + wc["recorded"] == wc["samples"]
    if "lut" in kw:
        assert sum(bool(plane.any()) for plane in want) >= 2
    if "depth" in kw:  # points in two slices at least, and points on the canvas that are dropped for their depth alone
        assert len(notes["slices"]) >= 2 and notes["dropped_for_depth"] > 0
        assert want.shape == ((3, h, w) if "lut" in kw else (kw["depth"][3], h, w))
    if "depth" in kw and "lut" in kw:  # a slice that receives points has a weight of zero
        assert any((plot.weights(kw["lut"])[s] == 0).any() for s in notes["slices"])
    assert cnt == wc
    assert hist.shape == want.shape and np.array_equal(hist, want)
    assert states.tobytes() == own.tobytes()
    assert int(hist.sum()) == cnt["increments"]


def test_the_plot_constant_comes_from_the_fixed_c(ref):
    """On the plane (c_re, c_im) every visited point lands on the pixel of the fixed c, whatever the sample."""
    c = (-0.8, 0.156)
    hist, cnt = plot.draw(ref, 64, 64, 200, 0, 8, [20], c=c, projection=((0, 0, 1, 0), (0, 0, 0, 1)))
    row, col = int((c[1] + 2.0) / 0.0625), int((c[0] + 2.0) / 0.0625)
    assert cnt["increments"] == cnt["replay_steps"] > 0
    assert int(hist[row, col]) == cnt["increments"] == int(hist.sum())


# ---- 2. the step is the power -----------------------------------------------------------------------------------------


def random_points(n, seed):
    """|z|^2 <= 8 (what a starting point can be; uniform over the disc), c in [-2, 2]^2."""
    rng = np.random.default_rng(seed)
    radius = math.sqrt(8.0) * np.sqrt(rng.uniform(0.0, 1.0, n))
    angle = rng.uniform(0.0, 2.0 * math.pi, n)
    c = rng.uniform(-2.0, 2.0, (n, 2))
    return [(float(a * math.cos(b)), float(a * math.sin(b)), float(x), float(y)) for a, b, (x, y) in zip(radius, angle, c)]


@pytest.mark.parametrize("degree", range(2, 9))
def test_step_is_z_to_the_d_plus_c(ref, degree):
    """Against z^d + c in exact rational arithmetic on the doubles.  Bound, per component: 64 * 2^-53 * (|z|^d + |c|) --
    each of the <= 7 complex multiplications contributes at most ~3 roundings' worth of relative error (one product, one
    fused sum, on magnitudes <= |z|^d), plus the addition of c: 7 * 3 + 1 = 22 units; 64 leaves a factor of two and the
    last power of two (the bound of tests/test_power_host.py, here from the starting points of a Julia render, and with degree 2)."""
    for r, i, cr, ci in random_points(500, 200 + degree):
        got_r, got_i, got_m = plot.step(ref, cr, ci, r, i, degree=degree)
        wr, wi = F(r), F(i)
        for _ in range(degree - 1):
            wr, wi = wr * F(r) - wi * F(i), wr * F(i) + wi * F(r)
        bound = 64.0 * 2.0 ** -53 * (math.hypot(r, i) ** degree + math.hypot(cr, ci))
        err_r, err_i = abs(F(got_r) - (wr + F(cr))), abs(F(got_i) - (wi + F(ci)))
        assert err_r <= F(bound) and err_i <= F(bound), (degree, r, i, cr, ci)
        assert got_m == float(F(got_i) * F(got_i) + F(got_r * got_r))  # the test value: fma of the new point
        assert (got_r, got_i, got_m) == py_step(cr, ci, r, i, degree)


def test_ship_step_takes_the_magnitudes(ref):
    for r, i, cr, ci in random_points(200, 77):
        assert plot.step(ref, cr, ci, r, i, ship=True) == plot.step(ref, cr, ci, abs(r), abs(i))
        assert plot.step(ref, cr, ci, r, i, ship=True) == py_step(cr, ci, r, i, ship=True)


# ---- 3. the OpenMP variant ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["z2_hologram", "d8"])
def test_result_does_not_depend_on_the_thread_count(ref, oracle, case):
    kw = {k: v for k, v in TINY[case].items() if k != "min_iter"}
    got = []
    for omp in (0, 4):
        states = oracle.init_states(1337, 0, 512)
        hist, cnt = plot.draw(ref, 333, 77, 300, 0, 512, [50, 7], box=(-1.6, 0.9, -0.7, 0.55), omp_threads=omp,
                              states=states, **kw)
        got.append((hist, cnt, states.tobytes()))
    assert got[0][1]["recorded"] > 100 and got[0][1]["increments"] > 100  # not empty
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- 4. the Python side ---------------------------------------------------------------------------------------------------


def test_names_in_header_and_package(cb, repo_root):
    import os

    import cudabrot_amd.capi as capi

    with open(os.path.join(repo_root, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    for name in ("cb_draw_buddhabrot_julia", "cb_renderer_set_julia", "cb_renderer_julia"):
        assert name + "(" in text and name in capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "Julia render" in text
    assert callable(cb.draw_buddhabrot_julia) and hasattr(cb.Renderer, "set_julia") and hasattr(cb.Renderer, "julia")
