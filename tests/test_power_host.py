"""The Multibrot render (include/cudabrot_amd.h, "Multibrot step") without a GPU: the CPU restatement
(tests/plot_reference.c) pinned to the oracle through its degree-2 driver without rejection, its step pinned to z^d + c
in exact rational arithmetic, and the Python side's constants."""

import ctypes as C
import math
from fractions import Fraction as F

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import ref  # noqa: F401


# ---- 1. the driver is the oracle's ------------------------------------------------------------------------------------

ANCHOR_CASES = {
    "64x64": (64, 64, (-2.0, 2.0, -2.0, 2.0)),
    "333x77": (333, 77, (-1.6, 0.9, -0.7, 0.55)),  # cropped, deltas no powers of two
}


@pytest.mark.parametrize("case", sorted(ANCHOR_CASES))
@pytest.mark.parametrize("omp", [0, 4])
def test_degree_2_driver_is_the_oracle_without_rejection(ref, oracle, case, omp):
    """Degree 2 with rejection switched off is the canonical z^2 + c step on every sample.  The oracle rejects the
    cardioid's and the bulb's samples unseen; where none of them would have escaped below max (asserted here, sample by sample), the two
    differ only in how they count them: never_escaped += rejected, iterate_steps += max * rejected."""
    w, h, box = ANCHOR_CASES[case]
    max_iter, min_iter, threads, launches = 500, 20, 1024, (50, 7)
    # the precondition: the oracle's rejected samples, from its own generator and shortcuts, iterated
    own = oracle.init_states(1337, 0, threads)
    rejected = 0
    for t in range(threads):
        g = oracle.Xorwow.from_buffer(own, t * own.dtype.itemsize)
        for _ in range(sum(launches)):
            cr = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            ci = oracle.lib.orc_uniform_double(C.byref(g)) * 4.0 - 2.0
            if oracle.lib.orc_in_main_cardioid(cr, ci) or oracle.lib.orc_in_order2_bulb(cr, ci):
                rejected += 1
                assert oracle.lib.orc_iterate_mandelbrot(cr, ci, max_iter) == max_iter, (cr, ci)
    want_states = oracle.init_states(1337, 0, threads)
    want_hist = np.zeros((h, w), dtype=np.uint64)
    want = dict.fromkeys(plot.COUNTER_NAMES, 0)
    for samples in launches:
        _, cnt = oracle.render(w, h, max_iter, min_iter, threads, 1, box=box, samples_per_thread=samples, hist=want_hist,
                               states=want_states)
        for name in want:
            want[name] += cnt[name]
    assert want["rejected"] == rejected > 1000 and want["recorded"] > 100 and want["increments"] > 1000
    states = oracle.init_states(1337, 0, threads)
    hist, cnt = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, reject=False, box=box, omp_threads=omp,
                          states=states)
    assert np.array_equal(hist, want_hist)
    assert states.tobytes() == want_states.tobytes() == own.tobytes()
    for name in ("samples", "too_fast", "recorded", "replay_steps", "increments"):
        assert cnt[name] == want[name], name
    assert cnt["rejected"] == 0
    assert cnt["never_escaped"] == want["never_escaped"] + want["rejected"]
    assert cnt["iterate_steps"] == want["iterate_steps"] + max_iter * want["rejected"]


# ---- 2. the step is the power -----------------------------------------------------------------------------------------


def random_points(n, seed):
    """|z| <= 2 (uniform over the disc), c in [-2, 2]^2 (|c| <= 2 sqrt 2)."""
    rng = np.random.default_rng(seed)
    radius = 2.0 * np.sqrt(rng.uniform(0.0, 1.0, n))
    angle = rng.uniform(0.0, 2.0 * math.pi, n)
    c = rng.uniform(-2.0, 2.0, (n, 2))
    return [(float(a * math.cos(b)), float(a * math.sin(b)), float(x), float(y)) for a, b, (x, y) in zip(radius, angle, c)]


@pytest.mark.parametrize("degree", range(3, 9))
def test_step_is_z_to_the_d_plus_c(ref, degree):
    """Against z^d + c in exact rational arithmetic on the doubles.  Bound, per component: 64 * 2^-53 * (|z|^d + |c|) --
    each of the <= 7 complex multiplications contributes at most ~3 roundings' worth of relative error (one product, one
    fused sum, on magnitudes <= |z|^d), plus the addition of c: 7 * 3 + 1 = 22 units; 64 is a factor two over that, with
    room for the last power of two."""
    worst = 0.0
    for r, i, cr, ci in random_points(1000, 100 + degree):
        got_r, got_i, _ = plot.step(ref, cr, ci, r, i, degree=degree)
        wr, wi = F(r), F(i)
        for _ in range(degree - 1):
            wr, wi = wr * F(r) - wi * F(i), wr * F(i) + wi * F(r)
        bound = 64.0 * 2.0 ** -53 * (math.hypot(r, i) ** degree + math.hypot(cr, ci))
        err_r, err_i = abs(F(got_r) - (wr + F(cr))), abs(F(got_i) - (wi + F(ci)))
        assert err_r <= F(bound) and err_i <= F(bound), (degree, r, i, cr, ci)
        worst = max(worst, float(max(err_r, err_i) / F(bound)))
    print("degree %d: largest error / bound = %.3f" % (degree, worst))


def test_degree_3_loop_is_the_step_written_out(ref):
    """The run-time loop against the two multiplications written out by hand, one rounding per operation, bit for bit."""

    def fma(a, b, c):
        return float(F(a) * F(b) + F(c))  # float(Fraction) rounds to nearest even: one rounding

    for r, i, cr, ci in random_points(1000, 3):
        t = i * i
        w2r = fma(r, r, -t)
        s = i * r
        w2i = fma(r, i, s)
        t = w2i * i
        w3r = fma(w2r, r, -t)
        s = w2i * r
        w3i = fma(w2r, i, s)
        nr, ni = cr + w3r, ci + w3i
        m = fma(ni, ni, nr * nr)
        got = plot.step(ref, cr, ci, r, i, degree=3)
        assert [x.hex() for x in got] == [nr.hex(), ni.hex(), m.hex()]


def test_escape_test_is_fma_of_the_new_point(ref):
    for degree in range(3, 9):
        for r, i, cr, ci in random_points(50, 50 + degree):
            nr, ni, m = plot.step(ref, cr, ci, r, i, degree=degree)
            assert m == float(F(ni) * F(ni) + F(nr * nr))


# ---- 3. the Python side -------------------------------------------------------------------------------------------------


def test_python_constants(cb):
    import cudabrot_amd.capi as capi

    assert (cb.CB_POWER_MIN, cb.CB_POWER_MAX, cb.CB_KERNEL_POWER_MASK) == (3, 8, 0xF000)
    assert [cb.CB_KERNEL_POWER(d) for d in range(3, 9)] == [0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000]
    assert capi.CB_KERNEL_POWER is cb.CB_KERNEL_POWER
    for d in range(3, 9):
        v = cb.CB_KERNEL_POWER(d)
        assert v & cb.CB_KERNEL_POWER_MASK == v and (v >> 12) == d
        assert v & (cb.CB_KERNEL_FLAG_BURNING_SHIP | cb.CB_KERNEL_FLAG_DRAIN | cb.CB_KERNEL_FLAG_ANTI | 0xFF) == 0
    for bad in (0, 1, 2, 9, 15, -1):
        with pytest.raises(ValueError):
            cb.CB_KERNEL_POWER(bad)


def test_header_states_the_same_constants(repo_root):
    import os
    import re

    with open(os.path.join(repo_root, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define CB_POWER_MIN 3\b", text) and re.search(r"#define CB_POWER_MAX 8\b", text)
    assert "#define CB_KERNEL_POWER(d) ((d) << 12)" in text and re.search(r"#define CB_KERNEL_POWER_MASK 0xF000\b", text)
    assert "Multibrot step" in text
