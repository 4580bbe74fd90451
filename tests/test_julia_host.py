"""The Julia render (include/cudabrot_amd.h, "Julia render") without a GPU: the CPU restatement (tests/julia_reference.c)
pinned to a pure-Python restatement of the definition on the oracle's generator, its step pinned to z^d + c in exact
rational arithmetic, and its independence of the OpenMP thread count."""

import ctypes as C
import math
from fractions import Fraction as F

import numpy as np
import pytest

import julia_reference as julia


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return julia.load(tmp_path_factory.mktemp("julia_ref"))


# ---- 1. the C restatement is the definition ---------------------------------------------------------------------------


def fma(a, b, c):
    """One rounding: math.fma where Python has it, else the exact rational value rounded to nearest even (all operands
    here are finite)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(F(a) * F(b) + F(c))


def py_step(degree, ship, cr, ci, r, i):
    """The step of the definition in Python's own IEEE doubles -> (r', i', |z'|^2)."""
    if degree == 2:
        ii = i * i
        t = fma(r, r, -ii)
        nr = cr + t
        ni = fma(abs(r) + abs(r), abs(i), ci) if ship else fma(r + r, i, ci)
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


def py_draw(oracle, w, h, box, max_iter, min_iter, threads, samples, c, degree, ship, p, states):
    """The definition, sample by sample, on the oracle's generator -> (hist, counters)."""
    d = oracle.make_dims(w, h, *box)
    hist = np.zeros((h, w), dtype=np.uint64)
    cnt = dict.fromkeys(julia.COUNTER_NAMES, 0)
    ku = fma(p[2], c[0], p[3] * c[1])
    kv = fma(p[6], c[0], p[7] * c[1])
    for t in range(threads):
        g = oracle.Xorwow.from_buffer(states, t * states.dtype.itemsize)
        for _ in range(samples):
            sr = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            si = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            cnt["samples"] += 1
            r, i, k = sr, si, max_iter
            for n in range(max_iter):
                r, i, m = py_step(degree, ship, c[0], c[1], r, i)
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
            r, i = sr, si
            for _ in range(k + 1):
                r, i, _ = py_step(degree, ship, c[0], c[1], r, i)
                cnt["replay_steps"] += 1
                u = fma(p[0], r, fma(p[1], i, ku))
                v = fma(p[4], r, fma(p[5], i, kv))
                if u < d.min_real or v < d.min_imag:
                    continue
                col, row = int((u - d.min_real) / d.delta_real), int((v - d.min_imag) / d.delta_imag)
                if 0 <= col < w and 0 <= row < h:
                    hist[row, col] += 1
                    cnt["increments"] += 1
    return hist, cnt


# (c, degree, ship, matrix): degree 2, the ship, the smallest and the largest Multibrot degree; one on another plane, so
# that K_u and K_v from the fixed c are part of what is compared
TINY = {
    "z2": ((-0.8, 0.156), 2, False, julia.IDENTITY),
    "z2_hologram": ((-0.8, 0.156), 2, False, julia.HOLOGRAM),
    "ship": ((-0.8, 0.156), 2, True, julia.IDENTITY),
    "d3": ((0.0, 0.0), 3, False, julia.IDENTITY),
    "d8": ((0.4, 0.2), 8, False, julia.IDENTITY),
}


@pytest.mark.parametrize("case", list(TINY))
def test_c_restatement_is_the_python_restatement(ref, oracle, case):
    c, degree, ship, p = TINY[case]
    w = h = 64
    box = (-2.0, 2.0, -2.0, 2.0)
    max_iter, min_iter, threads, samples = 200, 0 if degree == 8 else 2, 8, 20
    own = oracle.init_states(1337, 0, threads)
    want, wc = py_draw(oracle, w, h, box, max_iter, min_iter, threads, samples, c, degree, ship, julia.matrix(p), own)
    states = oracle.init_states(1337, 0, threads)
    hist, cnt = julia.draw(ref, w, h, max_iter, min_iter, threads, [samples], c, degree, ship, p, box=box, states=states)
    assert wc["samples"] == threads * samples and wc["rejected"] == 0
    assert wc["recorded"] > 0 and wc["increments"] > 0
    assert wc["never_escaped"] + wc["too_fast"] + wc["recorded"] == wc["samples"]
    assert cnt == wc
    assert np.array_equal(hist, want)
    assert states.tobytes() == own.tobytes()
    assert int(hist.sum()) == cnt["increments"]


def test_the_plot_constant_comes_from_the_fixed_c(ref):
    """On the plane (c_re, c_im) every visited point lands on the pixel of the fixed c, whatever the sample."""
    c = (-0.8, 0.156)
    hist, cnt = julia.draw(ref, 64, 64, 200, 0, 8, [20], c, projection=((0, 0, 1, 0), (0, 0, 0, 1)))
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
    last power of two (the bound of tests/test_power_host.py, here on the Julia restatement's own entry point)."""
    for r, i, cr, ci in random_points(500, 200 + degree):
        got_r, got_i, got_m = julia.step(ref, degree, False, cr, ci, r, i)
        wr, wi = F(r), F(i)
        for _ in range(degree - 1):
            wr, wi = wr * F(r) - wi * F(i), wr * F(i) + wi * F(r)
        bound = 64.0 * 2.0 ** -53 * (math.hypot(r, i) ** degree + math.hypot(cr, ci))
        err_r, err_i = abs(F(got_r) - (wr + F(cr))), abs(F(got_i) - (wi + F(ci)))
        assert err_r <= F(bound) and err_i <= F(bound), (degree, r, i, cr, ci)
        assert got_m == float(F(got_i) * F(got_i) + F(got_r * got_r))  # the test value: fma of the new point
        assert (got_r, got_i, got_m) == py_step(degree, False, cr, ci, r, i)


def test_ship_step_takes_the_magnitudes(ref):
    for r, i, cr, ci in random_points(200, 77):
        assert julia.step(ref, 2, True, cr, ci, r, i) == julia.step(ref, 2, False, cr, ci, abs(r), abs(i))
        assert julia.step(ref, 2, True, cr, ci, r, i) == py_step(2, True, cr, ci, r, i)


# ---- 3. the OpenMP variant ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["z2_hologram", "d8"])
def test_result_does_not_depend_on_the_thread_count(ref, oracle, case):
    c, degree, ship, p = TINY[case]
    got = []
    for omp in (0, 4):
        states = oracle.init_states(1337, 0, 512)
        hist, cnt = julia.draw(ref, 333, 77, 300, 0, 512, [50, 7], c, degree, ship, p, box=(-1.6, 0.9, -0.7, 0.55),
                               omp_threads=omp, states=states)
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
