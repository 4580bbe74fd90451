"""The formula step (include/cudabrot_amd.h, "Formula step") without a GPU: the restatement's five steps
(tests/plot_reference.c) against its plain and Burning Ship steps through the identities that define the family, bit
for bit -- two settings of the one step function, a formula code against PLAIN (code 0) or SHIP (code 0 with the ship
flag); the header's text and constants; the Python constants."""

import os
import re
import struct

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import ref  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, C, B, P, CT = (plot.NAMES[n] for n in ("tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn"))


def step(ref, f, cr, ci, r, i):
    return plot.step(ref, cr, ci, r, i, formula=f)


def bits(x):
    return struct.pack("<d", x)


def same(a, b):
    """Two step results (r', i', m), bit for bit: -0.0 is not +0.0."""
    return all(bits(x) == bits(y) for x, y in zip(a, b))


def inputs():
    """(cr, ci, r, i): random points of the disc the iteration lives in, points with |z| near 2, and the edge values
    -- signed zeros, subnormals, the smallest normals -- in every coordinate."""
    rng = np.random.default_rng(20240518)
    out = [tuple(v) for v in rng.uniform(-2.0, 2.0, size=(3000, 4))]
    for _ in range(1000):  # |z| near 2: within a few ulps to a few percent, either side
        angle = rng.uniform(0.0, 2.0 * np.pi)
        radius = 2.0 * (1.0 + rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-16.0, -1.5))
        out.append((rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0), radius * np.cos(angle), radius * np.sin(angle)))
    edge = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 2.0, -2.0,
            1.4142135623730951, -1.4142135623730951]
    for r in edge:
        for i in edge:
            for c in ((0.0, 0.0), (-0.0, -0.0), (0.3, -0.7), (5e-324, -5e-324), (-2.0, 2.0)):
                out.append((c[0], c[1], r, i))
    return [tuple(float(x) for x in v) for v in out]


INPUTS = inputs()


def test_enough_inputs_on_both_sides_of_t():
    t = [r * r - i * i for _, _, r, i in INPUTS]
    assert len(INPUTS) > 4000 and sum(x > 0 for x in t) > 1000 and sum(x < 0 for x in t) > 1000


def test_tricorn_is_the_plain_step_of_the_conjugate(ref):
    for cr, ci, r, i in INPUTS:
        assert same(step(ref, T, cr, ci, r, i), step(ref, plot.PLAIN, cr, ci, r, -i)), (cr, ci, r, i)


def test_perpendicular_is_the_plain_step_of_minus_abs_r(ref):
    for cr, ci, r, i in INPUTS:
        assert same(step(ref, P, cr, ci, r, i), step(ref, plot.PLAIN, cr, ci, -abs(r), i)), (cr, ci, r, i)


def test_celtic_is_plain_and_buffalo_is_ship_where_t_is_not_negative(ref):
    seen = 0
    for cr, ci, r, i in INPUTS:
        t = step(ref, plot.PLAIN, 0.0, 0.0, r, i)[0]  # nr = 0 + t: the step's own rounded t (a -0 reads +0)
        if not t >= 0.0 or bits(t) == bits(-0.0):
            continue
        seen += 1
        assert same(step(ref, C, cr, ci, r, i), step(ref, plot.PLAIN, cr, ci, r, i)), (cr, ci, r, i)
        assert same(step(ref, B, cr, ci, r, i), step(ref, plot.SHIP, cr, ci, r, i)), (cr, ci, r, i)
    assert seen > 1000


def test_celtic_and_buffalo_differ_from_them_where_t_is_negative(ref):
    differ = 0
    for cr, ci, r, i in INPUTS[:3000]:
        if r * r - i * i < -0.01:
            differ += not same(step(ref, C, cr, ci, r, i), step(ref, plot.PLAIN, cr, ci, r, i))
            assert step(ref, C, cr, ci, r, i)[1:2] == step(ref, plot.PLAIN, cr, ci, r, i)[1:2]  # ni is
    assert differ > 500


def test_celtic_tricorn_is_celtic_of_the_conjugate(ref):
    for cr, ci, r, i in INPUTS:
        assert same(step(ref, CT, cr, ci, r, i), step(ref, C, cr, ci, r, -i)), (cr, ci, r, i)


def test_the_five_steps_are_five_different_maps(ref):
    # both signs of r, of i and of t: every sign and magnitude in the table shows on some point
    points = [(sr * a, si * b) for a, b in ((0.6, 0.9), (0.9, 0.6)) for sr in (1, -1) for si in (1, -1)]
    maps = {tuple(step(ref, f, 0.3, -0.2, r, i) for r, i in points)
            for f in (plot.PLAIN, plot.SHIP, T, C, B, P, CT)}
    assert len(maps) == 7


# ---- the header and the Python constants ------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        return f.read()


def defined(header, name):
    m = re.search(r"^#define %s\s+(\S+)" % re.escape(name), header, re.M)
    assert m, name
    return int(m.group(1), 0)


CODES = {"CB_FORMULA_TRICORN": 1, "CB_FORMULA_CELTIC": 2, "CB_FORMULA_BUFFALO": 3, "CB_FORMULA_PERPENDICULAR": 4,
         "CB_FORMULA_CELTIC_TRICORN": 5, "CB_FORMULA_MAX": 5}


def test_header_constants(header):
    for name, value in CODES.items():
        assert defined(header, name) == value
    assert re.search(r"^#define CB_KERNEL_FORMULA\(f\) \(\(f\) << 16\)$", header, re.M)
    mask = defined(header, "CB_KERNEL_FORMULA_MASK")
    assert mask == 0xF0000
    assert [f << 16 for f in range(1, 6)] == [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]
    assert all((f << 16) & mask == f << 16 for f in range(1, 6))
    others = [defined(header, n) for n in ("CB_KERNEL_FLAG_BURNING_SHIP", "CB_KERNEL_FLAG_DRAIN", "CB_KERNEL_FLAG_ANTI",
                                           "CB_KERNEL_POWER_MASK")]
    others += [defined(header, n) for n in ("CB_KERNEL_DEFAULT", "CB_KERNEL_SIMPLE", "CB_KERNEL_TIMED",
                                            "CB_KERNEL_FULL_ITERATE")]
    assert others[:4] == [0x100, 0x200, 0x400, 0xF000]
    for v in others:
        assert v & mask == 0, hex(v)
    assert defined(header, "CB_ABI_VERSION") == 1  # the change only adds


def test_header_text(header):
    start = header.index("Formula step: tricorn, Celtic and kin")
    assert header.index("Multibrot step: z^d + c") < start < header.index("CB_ERROR_FOCUS_EMPTY 100002")
    text = header[start:header.index("#define CB_FORMULA_TRICORN")]
    flat = " ".join(text.replace("*", " ").split())
    for row in ("1 tricorn cr + t fma(-(r + r), i, ci)", "2 celtic cr + fabs(t) fma(r + r, i, ci)",
                "3 buffalo cr + fabs(t) fma(fabs(r) + fabs(r), fabs(i), ci)",
                "4 perpendicular cr + t fma(-(fabs(r) + fabs(r)), i, ci)",
                "5 celtic-tricorn cr + fabs(t) fma(-(r + r), i, ci)"):
        assert row in flat, row
    for phrase in ("ii = i i", "t = fma(r, r, -ii)", "m = fma(ni, ni, nr nr)", "rejected = 0", "no interior map",
                   "Every visited point is finite", "4 + 2 sqrt(2)", "hipErrorInvalidValue"):
        assert phrase in flat, phrase
    assert "16 the formula product kernel" in " ".join(header.replace("*", " ").split())


def test_python_constants():
    from cudabrot_amd import capi

    for name, value in CODES.items():
        assert getattr(capi, name) == value
    assert capi.CB_KERNEL_FORMULA_MASK == 0xF0000
    assert [capi.CB_KERNEL_FORMULA(f) for f in range(1, 6)] == [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]
    assert capi.CB_FORMULA_NAMES == plot.NAMES
    for name, code in plot.NAMES.items():
        assert capi.CB_KERNEL_FORMULA(name) == code << 16
    for bad in (0, 6, -1, 16, "mandelbrot", "Tricorn"):
        with pytest.raises(ValueError):
            capi.CB_KERNEL_FORMULA(bad)
    import cudabrot_amd

    assert cudabrot_amd.CB_KERNEL_FORMULA is capi.CB_KERNEL_FORMULA and cudabrot_amd.CB_FORMULA_MAX == 5
