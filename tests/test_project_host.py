"""The projected render (include/cudabrot_amd.h, "Projected render") without a GPU: the CPU restatement
(tests/plot_reference.c) pinned to the oracle through the identity matrix, and to an independent count through the
c-plane."""

import ctypes as C

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import ref  # noqa: F401


# (w, h, box, max_iter, min_iter, threads, passes, ship): a dyadic canvas, a 333 x 77 one, a cropped Burning Ship
IDENTITY_CASES = {
    "dyadic": (256, 256, (-2.0, 2.0, -2.0, 2.0), 300, 10, 96, 2, False),
    "333x77": (333, 77, (-2.0, 2.0, -2.0, 2.0), 200, 5, 80, 2, False),
    "ship": (200, 120, (-2.2, 1.4, -2.0, 0.9), 150, 8, 64, 2, True),
}


@pytest.mark.parametrize("case", sorted(IDENTITY_CASES))
@pytest.mark.parametrize("omp", [0, 4])
def test_identity_matrix_is_the_oracle(ref, oracle, case, omp):
    w, h, box, max_iter, min_iter, threads, passes, ship = IDENTITY_CASES[case]
    want_states = oracle.init_states(1337, 0, threads)
    want_hist, want_cnt = oracle.render(w, h, max_iter, min_iter, threads, passes, box=box, states=want_states,
                                        burning_ship=ship)
    states = oracle.init_states(1337, 0, threads)
    hist, cnt = plot.draw(ref, w, h, max_iter, min_iter, threads, [50] * passes, projection=plot.IDENTITY, box=box, ship=ship,
                          omp_threads=omp, states=states)
    assert want_cnt["increments"] > 0 and want_cnt["recorded"] > 0
    assert np.array_equal(hist, want_hist)
    assert states.tobytes() == want_states.tobytes()
    assert cnt == want_cnt


def test_plane_zr_zi_is_the_identity():
    assert np.array_equal(plot.plane("zr", "zi"), np.array(plot.IDENTITY))
    assert np.array_equal(plot.plane("cr", "ci"), np.array(plot.C_PLANE))
    assert np.array_equal(plot.plane("zr", "cr"), np.array(plot.ZR_CR))


def test_c_plane_puts_the_whole_orbit_on_the_pixel_of_c(ref, oracle):
    """With P = {{0,0,1,0},{0,0,0,1}} every visited point of a sample is plotted at c itself: an accepted sample with c
    on the canvas adds exactly k + 1 to the single pixel of c.  Counted here sample by sample from the oracle's generator,
    shortcuts and IterateMandelbrot, with the pixel taken in Python's own double arithmetic."""
    w = h = 64
    box = (-1.5, 0.5, -1.0, 1.0)  # cropped: some accepted samples lie outside
    max_iter, min_iter, threads, samples = 400, 3, 48, 50
    d = oracle.make_dims(w, h, *box)
    want = np.zeros((h, w), dtype=np.uint64)
    recorded = off_canvas = 0
    st = oracle.init_states(1337, 0, threads)
    own = st.copy()
    for t in range(threads):
        g = oracle.Xorwow.from_buffer(own, t * own.dtype.itemsize)
        for _ in range(samples):
            cr = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            ci = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            if oracle.lib.orc_in_main_cardioid(cr, ci) or oracle.lib.orc_in_order2_bulb(cr, ci):
                continue
            k = oracle.lib.orc_iterate_mandelbrot(cr, ci, max_iter)
            if k >= max_iter or k < min_iter:
                continue
            recorded += 1
            if cr < d.min_real or ci < d.min_imag:
                off_canvas += 1
                continue
            col, row = int((cr - d.min_real) / d.delta_real), int((ci - d.min_imag) / d.delta_imag)
            if 0 <= col < w and 0 <= row < h:
                want[row, col] += k + 1
            else:
                off_canvas += 1
    hist, cnt = plot.draw(ref, w, h, max_iter, min_iter, threads, [samples], projection=plot.C_PLANE, box=box, states=st)
    assert recorded > 50 and off_canvas > 0
    assert cnt["recorded"] == recorded
    assert np.array_equal(hist, want)
    assert int(hist.sum()) == cnt["increments"]
    assert st.tobytes() == own.tobytes()


def test_a_general_point_is_four_fused_operations(ref):
    """plot_point against the definition written out in exact rational arithmetic, rounded once per operation."""
    from fractions import Fraction as F

    def fma(a, b, c):
        return float(F(a) * F(b) + F(c))  # float(Fraction) rounds to nearest even: one rounding

    rng = np.random.default_rng(7)
    for _ in range(200):
        p = rng.uniform(-2.0, 2.0, 8)
        zr, zi, cr, ci = rng.uniform(-2.0, 2.0, 4)
        u, v = plot.point(ref, p, zr, zi, cr, ci)
        ku = fma(p[2], cr, float(F(p[3]) * F(ci)))
        kv = fma(p[6], cr, float(F(p[7]) * F(ci)))
        assert u == fma(p[0], zr, fma(p[1], zi, ku))
        assert v == fma(p[4], zr, fma(p[5], zi, kv))


def test_hologram_matrix_is_a_pair_of_orthonormal_rows():
    p = np.array(plot.HOLOGRAM)
    assert np.allclose(p @ p.T, np.eye(2), atol=1e-15)
    nonzero = p[p != 0.0]
    assert nonzero.size == 4 and not np.any(nonzero == np.round(nonzero))  # irrational entries, none exact
