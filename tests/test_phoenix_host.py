"""The Phoenix render (include/cudabrot_amd.h, "Phoenix render") without a GPU: the step of its CPU restatement
(tests/phoenix_reference.c) against hand-derived values and against the definition in Python's own doubles, the
restatement with p = 0 against the plotted renders' restatement (the section's two Consequences), the discounts' rule, and
the new names in the header and the package."""

import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import phoenix_reference as phoenix
import plot_reference as plot
from plot_harness import ref  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = float.fromhex


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return phoenix.load(tmp_path_factory.mktemp("phoenix_ref"))


def fma(a, b, c):
    """One rounding: math.fma where Python has it, else the exact rational value rounded to nearest even."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(F(a) * F(b) + F(c))


def py_step(cr, ci, p_re, p_im, r, i, y_re, y_im):
    """The section's operation sequence in Python's own IEEE doubles."""
    ii = i * i
    t = fma(r, r, -ii)
    nr = cr + t
    ni = fma(r + r, i, ci)
    nr = fma(p_re, y_re, nr)
    nr = fma(-p_im, y_im, nr)
    ni = fma(p_re, y_im, ni)
    ni = fma(p_im, y_re, ni)
    return nr, ni, r, i, fma(ni, ni, nr * nr)


# (c, p, z, y) -> (z', y', |z'|^2), derived by hand:
#  1. dyadic data, every operation exact: z^2 + c = 2.25 + i, p y = (0.5 - 0.25 i)(2 - i) = 0.75 - i, the sum 3
#  2. p_re y_re = (1 + 2^-27)^2 = 1 + 2^-26 + 2^-54 fused into nr = -1: 2^-26 + 2^-54 (a product rounded first gives
#     2^-26); |z'|^2 = 2^-52 (1 + 2^-27 + 2^-56) rounds to 2^-52 (1 + 2^-27)
#  3. -p_im y_im = -(1 + 2^-27)^2 fused into nr = 0: rounds to -(1 + 2^-26), the square of which, 1 + 2^-25 + 2^-52, is
#     exact; the negation is p_im's, not the product's
KNOWN = [
    ((0.25, -0.5), (0.5, -0.25), (1.5, 0.5), (2.0, -1.0), (3.0, 0.0), (1.5, 0.5), 9.0),
    ((-1.0, 0.0), (H("0x1.0000002p+0"), 0.0), (0.0, 0.0), (H("0x1.0000002p+0"), 0.0), (H("0x1.0000001p-26"), 0.0),
     (0.0, 0.0), H("0x1.0000002p-52")),
    ((0.0, 0.0), (0.0, H("0x1.0000002p+0")), (0.0, 0.0), (0.0, H("0x1.0000002p+0")), (H("-0x1.0000004p+0"), 0.0),
     (0.0, 0.0), H("0x1.0000008000001p+0")),
]


@pytest.mark.parametrize("c,p,z,y,z1,y1,m1", KNOWN)
def test_step_against_hand_derived_values(pref, c, p, z, y, z1, y1, m1):
    r, i, yr, yi, m = phoenix.step(pref, *c, *p, *z, *y)
    assert (r, i) == z1 and (yr, yi) == y1 and m == m1, ((r.hex(), i.hex()), (yr, yi), m.hex())


def test_step_is_the_sections_sequence_on_random_states(pref):
    rng = np.random.default_rng(5)
    for _ in range(2000):
        c, p, z, y = (tuple(float(v) for v in rng.uniform(-2.0, 2.0, 2)) for _ in range(4))
        r, i, yr, yi, m = phoenix.step(pref, *c, *p, *z, *y)
        want = py_step(*c, *p, *z, *y)
        assert [v.hex() for v in (r, i, yr, yi, m)] == [v.hex() for v in want]


def test_p_zero_step_is_mandel_step_up_to_the_sign_of_a_zero(pref, ref):  # noqa: F811
    rng = np.random.default_rng(6)
    for _ in range(500):
        c, z, y = (tuple(float(v) for v in rng.uniform(-2.0, 2.0, 2)) for _ in range(3))
        r, i, yr, yi, m = phoenix.step(pref, *c, 0.0, 0.0, *z, *y)
        assert (r, i, m) == plot.step(ref, *c, *z) and (yr, yi) == z


SHAPE = dict(w=32, h=24, max_iter=200, min_iter=5, n_threads=96, launches=(3, 2))


def both(pref, ref, oracle, **kw):  # noqa: F811
    """The Phoenix restatement with p = 0 and plot_reference.draw with the same arguments, each on generators of its own."""
    s = dict(SHAPE)
    args = (s.pop("w"), s.pop("h"), s.pop("max_iter"), s.pop("min_iter"), s.pop("n_threads"), s.pop("launches"))
    st_a, st_b = oracle.init_states(1337, 0, args[4]), oracle.init_states(1337, 0, args[4])
    got = phoenix.draw(pref, *args, p=(0.0, 0.0), states=st_a, **{k: v for k, v in kw.items() if k != "reject"})
    want = plot.draw(ref, *args, states=st_b, **kw)
    return got, want, st_a, st_b


@pytest.mark.parametrize("projection", [plot.IDENTITY, plot.HOLOGRAM], ids=["identity", "hologram"])
def test_p_zero_with_a_fixed_c_is_the_julia_render(pref, ref, oracle, projection):  # noqa: F811
    (hist, cnt), (want, wc), st_a, st_b = both(pref, ref, oracle, c=(-0.8, 0.156), projection=projection)
    assert cnt == wc and cnt["recorded"] > 0 and cnt["never_escaped"] > 0 and cnt["increments"] > 0
    assert np.array_equal(hist, want) and st_a.tobytes() == st_b.tobytes()


@pytest.mark.parametrize("projection", [plot.IDENTITY, plot.ZR_CR], ids=["identity", "zr_cr"])
def test_p_zero_with_a_sampled_c_is_the_projected_render_without_rejection(pref, ref, oracle, projection):  # noqa: F811
    (hist, cnt), (want, wc), st_a, st_b = both(pref, ref, oracle, reject=False, projection=projection)
    assert cnt == wc and cnt["rejected"] == 0 and cnt["recorded"] > 0 and cnt["never_escaped"] > 0
    assert np.array_equal(hist, want) and st_a.tobytes() == st_b.tobytes()


def test_openmp_workers_do_not_change_the_restatement(pref):
    a = phoenix.draw(pref, 32, 24, 200, 5, 96, (3, 2), p=(-0.5, 0.0), omp_threads=0)
    b = phoenix.draw(pref, 32, 24, 200, 5, 96, (3, 2), p=(-0.5, 0.0), omp_threads=4)
    assert a[1] == b[1] and np.array_equal(a[0], b[0])


def test_discounts_follow_the_rule(pref):
    """A z-only comparison finds whatever the state comparison finds, no later; below the first comparison (the save after
    chunk one, the test after chunk two: max <= 120) there is nothing to discount; and the discounts are no part of the
    definition's counters."""
    extra = {}
    _, cnt = phoenix.draw(pref, 32, 24, 500, 20, 256, (20,), p=(-0.5, 0.0), extra=extra)
    assert extra["cycles_z_only"] >= extra["cycles_state"] > 0
    assert extra["skipped_z_only"] >= extra["skipped_state"] > 0
    assert extra["cycles_state"] <= cnt["never_escaped"] and extra["skipped_state"] < 500 * cnt["never_escaped"]
    assert set(cnt) == set(plot.COUNTER_NAMES)
    for max_iter in (60, 61, 120):
        extra = {}
        phoenix.draw(pref, 32, 24, max_iter, 5, 256, (20,), p=(-0.5, 0.0), extra=extra)
        assert extra == dict.fromkeys(phoenix.EXTRA_NAMES, 0), (max_iter, extra)
    extra = {}
    # max 181: the comparisons below max are at k = 120 (with the point of k = 60) and k = 180 (with that of k = 120), so
    # whatever is found discounts 61 steps or one.  (An attracting fixed point of this p contracts by sqrt |p| = 0.71 a
    # step: 1e-9 after 60 steps, 1e-18 after 120 -- an orbit is on its exact cycle at k = 120 at the earliest.)
    phoenix.draw(pref, 32, 24, 181, 5, 256, (20,), p=(-0.5, 0.0), extra=extra)
    print(extra)
    late = extra["skipped_state"] - 61 * extra["cycles_state"]  # = -60 * (found at k = 180)
    assert late % 60 == 0 and 0 <= -late // 60 <= extra["cycles_state"]


def test_header_and_package_define_the_new_names(cb):
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        header = f.read()
    assert int(re.search(r"#define CB_ABI_VERSION (\d+)", header).group(1)) == 1 == cb.lib.cb_abi_version()  # only adds
    assert "Phoenix render: a step with memory" in header
    for name in ("cb_draw_buddhabrot_phoenix", "cb_renderer_set_phoenix", "cb_renderer_phoenix"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in cb.capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "24 the Phoenix product kernel" in header and "25 the Phoenix lock-step kernel" in header
    assert "draw_buddhabrot_phoenix" in cb.__all__ and callable(cb.draw_buddhabrot_phoenix)
    assert hasattr(cb.Renderer, "set_phoenix") and hasattr(cb.Renderer, "phoenix")
