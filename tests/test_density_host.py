"""The density filter on the host (include/cudabrot_amd.h, "Density filter"), without a GPU:
cb_density_thresholds and cb_density_filter against the restatement in Python integers (tests/density_reference.py), the
three consequences the definition names asserted directly, and the refusals."""

import ctypes as C

import numpy as np
import pytest

import density_reference as dens

INVALID = 1  # hipErrorInvalidValue
CASES = dens.cases()


def test_thresholds_of_the_header(cb):
    assert cb.density_thresholds(8, 0.5, 1)[1:] == [64, 16, 7, 4, 2, 1, 1, 1]
    assert cb.density_thresholds(4, 0.4, 16)[1:] == [512, 90, 32, 16]
    assert cb.density_thresholds(4, 0.5, 9)[1:] == [144, 36, 16, 9]
    assert dens.thresholds(8, 1.0 / 16.0, 1) is None
    with pytest.raises(cb.CudabrotError):
        cb.density_thresholds(8, 1.0 / 16.0, 1)
    assert cb.CB_DENSITY_MAX_RADIUS == dens.MAX_RADIUS == 8


def test_thresholds_equal_the_restatement_on_a_grid(cb):
    refused = 0
    for radius in range(1, 9):
        for alpha in (1.0 / 16.0, 0.1, 0.25, 0.4, 0.5, 1.0 / 3.0, 0.7, 1.0, 1.5, float.fromhex("0x1.999999999999ap-1"), 4.0):
            for n0 in (1, 2, 3, 9, 16, 1000, 65_537, 1 << 20):
                want = dens.thresholds(radius, alpha, n0)
                table = (C.c_uint64 * (radius + 1))(*([77] * (radius + 1)))
                rc = cb.lib.cb_density_thresholds(radius, alpha, n0, table)
                if want is None:
                    refused += 1
                    assert rc == INVALID and list(table) == [77] * (radius + 1), (radius, alpha, n0)
                    continue
                assert rc == 0 and list(table) == want, (radius, alpha, n0)
                assert want[0] == (1 << 64) - 1 and want[radius] == n0 and want[1] < 1 << 22
                assert all(want[r] >= want[r + 1] for r in range(radius))
    assert refused > 0


def test_thresholds_refuse_parameters_out_of_range(cb):
    table = (C.c_uint64 * 9)(*([77] * 9))
    f = cb.lib.cb_density_thresholds
    for radius, alpha, n0 in [(0, 0.5, 1), (9, 0.5, 1), (-1, 0.5, 1), (4, 0.0625 - 1e-9, 1), (4, 4.0 + 1e-9, 1), (4, float("nan"), 1),
                              (4, float("inf"), 1), (4, -0.5, 1), (4, 0.5, 0), (4, 0.5, (1 << 20) + 1),
                              (8, 0.5, 1 << 16),   # T[1] = 2^22 exactly
                              (8, 0.0625, 1 << 20)]:  # floor(...) passes 2^64: decided before any conversion
        assert f(radius, alpha, n0, table) == INVALID, (radius, alpha, n0)
        assert dens.thresholds(radius, alpha, n0) is None
    assert f(4, 0.5, 1, None) == INVALID
    assert list(table) == [77] * 9
    assert f(8, 0.5, (1 << 16) - 1, table) == 0 and table[1] == 64 * ((1 << 16) - 1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_filter_equals_the_restatement(cb, name):
    hist, group, params = CASES[name]
    table = cb.density_thresholds(*params)
    assert table == dens.thresholds(*params)
    got = cb.density_filter(hist, table, group)
    assert got.dtype == np.uint64 and got.shape == hist.shape
    assert np.array_equal(got, dens.expected(name))


def test_the_impulse_of_the_header(cb):
    out = cb.density_filter(dens.impulse(), cb.density_thresholds(4, 0.5, 1))
    rows = [[0] * 9] + dens.IMPULSE_ROWS + dens.IMPULSE_ROWS[2::-1] + [[0] * 9]
    assert out.tolist() == rows


def test_the_cases_hold_what_they_are_named_for(cb):
    t = dens.thresholds(4, 0.5, 9)
    g = dens.group_of_three()
    assert dens.radius_of(21, t) == 2 and dens.radius_of(7, t) == 4      # the key crosses thresholds no plane crosses
    together, apart = dens.expected("group_of_three"), dens.expected("group_of_three_apart")
    assert not np.array_equal(together, apart)
    assert together[0, 5, 2] == 0 and apart[0, 5, 1] > 0                  # radius 2 against radius 4
    assert not together[0, :, 14:].any() and not together[2, :, 14:].any() and together[1, 2, 17] > 0  # empty planes stay empty
    assert np.array_equal(g[0, :, :14], g[1, :, :14]) and np.array_equal(together[0, :, :14], together[1, :, :14])
    four = dens.expected("four_planes")
    assert four[0, 9, 4] > 0 and four[1, 0, 6] > 0 and not four[2].any()
    for p in range(4):  # no plane bleeds into the next: each comes out as it does alone
        assert np.array_equal(four[p], dens.density_filter(dens.four_planes()[p], dens.thresholds(*dens.DEFAULT)))
    huge = dens.expected("huge_beside_one")
    assert int(huge[3, 3]) == (1 << 62) + int(dens.expected("impulse")[4, 3])  # sharp, plus its neighbour's blob
    assert not dens.expected("all_zero").any()
    # at the thresholds: T[r] has radius r, T[r] + 1 radius r - 1
    for params in ((4, 0.4, 16), (8, 0.5, 1)):
        t = dens.thresholds(*params)
        for r in range(1, len(t)):
            if r == len(t) - 1 or t[r] > t[r + 1]:
                assert dens.radius_of(t[r], t) == r
            assert dens.radius_of(t[r] + 1, t) < r


def test_counters_above_every_threshold_come_out_shifted(cb):
    table = cb.density_thresholds(4, 0.5, 4)  # T[1] = 64
    hist = dens.heavy_tail(9, 23, 31, scale=400.0)
    hist[(hist > 0) & (hist <= 64)] = 65
    assert np.count_nonzero(hist) > 300 and int(hist[hist > 0].min()) == 65
    out = cb.density_filter(hist, table)
    assert np.array_equal(out, hist << np.uint64(8))
    rgb = np.stack([hist, np.zeros_like(hist), np.zeros_like(hist)])
    assert np.array_equal(cb.density_filter(rgb, table, group=3), rgb << np.uint64(8))


def test_the_mass_is_conserved_up_to_the_final_floor(cb):
    radius, n0 = 4, 4
    table = cb.density_thresholds(radius, 0.5, n0)
    hist = dens.heavy_tail(5, 23, 31)
    hist[:radius] = hist[-radius:] = 0
    hist[:, :radius] = hist[:, -radius:] = 0
    assert {dens.radius_of(int(c), table) for c in hist[hist > 0]} == {0, 1, 2, 3, 4}  # all five radii occur
    out = cb.density_filter(hist, table)
    deficit = 256 * int(hist.sum(dtype=np.uint64)) - int(out.sum(dtype=np.uint64))
    assert 0 <= deficit < hist.size, deficit
    assert deficit > 0  # the floor does lose something on this array
    assert np.array_equal(out, dens.density_filter(hist, table))


def test_the_result_depends_on_no_order(cb):
    """A flipped input gives the flipped output (the kernel is symmetric): whatever order an implementation adds in."""
    hist, _, params = CASES["heavy_tail_8_0.5_1"]
    table = cb.density_thresholds(*params)
    out = cb.density_filter(hist, table)
    assert np.array_equal(cb.density_filter(hist[::-1, ::-1], table), out[::-1, ::-1])
    assert np.array_equal(cb.density_filter(hist.T, table), out.T)


def raw_filter(cb, hist, w, h, planes, group, table, out):
    t = (C.c_uint64 * len(table))(*table)
    return cb.lib.cb_density_filter(hist, w, h, planes, group, len(table) - 1, t, out)


def test_filter_refusals_leave_the_output_untouched(cb):
    table = dens.thresholds(4, 0.5, 1)
    hist = dens.huge_beside_one()
    out = np.full(hist.shape, 77, dtype=np.uint64)
    assert raw_filter(cb, hist.ctypes.data, 8, 8, 1, 1, table, out.ctypes.data) == 0 and int(out[3, 3]) >= 1 << 62
    out[:] = 77
    hist[7, 7] = 1 << 55   # a counter of 2^55, behind everything else
    assert raw_filter(cb, hist.ctypes.data, 8, 8, 1, 1, table, out.ctypes.data) == INVALID
    assert dens.density_filter(hist, table) is None
    hist[7, 7] = (1 << 55) - 1
    assert raw_filter(cb, hist.ctypes.data, 8, 8, 1, 1, table, out.ctypes.data) == 0
    out[:] = 77
    a = hist.ctypes.data
    bad_tables = [[0] + table[1:], table[:1] + [1 << 22] + table[2:], [table[0], 4, 16, 2, 1], table[:4] + [0]]
    calls = [(None, 8, 8, 1, 1, table, out.ctypes.data), (a, 8, 8, 1, 1, table, None), (a, 0, 8, 1, 1, table, out.ctypes.data),
             (a, 8, -1, 1, 1, table, out.ctypes.data), (a, 8, 8, 0, 1, table, out.ctypes.data),
             (a, 8, 8, 1, 2, table, out.ctypes.data), (a, 8, 8, 1, 3, table, out.ctypes.data),   # 3 does not divide 1
             (a, 8, 8, 1, 0, table, out.ctypes.data)] + [(a, 8, 8, 1, 1, t, out.ctypes.data) for t in bad_tables]
    for call in calls:
        assert raw_filter(cb, *call) == INVALID, call
    assert (out == 77).all()
    # aliasing: in place, and overlapping by one counter from either side
    both = np.zeros(2 * 64 - 1, dtype=np.uint64)
    both[:] = 1
    base = both.ctypes.data
    for src, dst in ((base, base), (base, base + 8 * 63), (base + 8 * 63, base)):
        assert raw_filter(cb, src, 8, 8, 1, 1, table, dst) == INVALID
    assert (both == 1).all()
    assert cb.lib.cb_density_arguments_ok(base, 8, 8, 1, 1, 4, (C.c_uint64 * 5)(*table), base + 8 * 64) == 1
