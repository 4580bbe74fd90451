"""The equalised image on the host (include/cudabrot_amd.h, "Equalised image"), without a GPU: the key at
its edges, cb_equalize_bins, cb_equalize_table and cb_set_grayscale_pixels_equalized against the restatement in Python
integers (tests/equalize_reference.py), the consequences of the definition asserted directly, and the refusals."""

import ctypes as C

import numpy as np
import pytest

import equalize_reference as eq

INVALID = 1  # hipErrorInvalidValue
CASES = eq.cases()


def test_key_values_at_the_edges_and_monotone(cb):
    assert cb.CB_EQUALIZE_KEYS == eq.KEYS == 56320
    for c, k in eq.KEY_ANCHORS.items():
        assert cb.equalize_key(c) == k == eq.key(c), c
    for k in range(10, 64):  # around every power of two the key moves by 0 or 1
        around = [cb.equalize_key(c) for c in range((1 << k) - 2, (1 << k) + 3) if c < 1 << 64]
        assert around == [eq.key(c) for c in range((1 << k) - 2, (1 << k) + 3) if c < 1 << 64]
        assert all(b - a in (0, 1) for a, b in zip(around, around[1:])), k
    rng = np.random.default_rng(1)
    sample = np.sort(rng.integers(0, 1 << 63, size=4000, dtype=np.uint64) >> rng.integers(0, 63, size=4000).astype(np.uint64))
    keys = [cb.equalize_key(int(c)) for c in sample]
    assert keys == [eq.key(int(c)) for c in sample] and keys == sorted(keys)
    for k in range(eq.KEYS):  # each key's lowest count maps back to it, and the count below it to the key below
        low = eq.lowest_count(k)
        assert cb.equalize_key(low) == k and (k == 0 or cb.equalize_key(low - 1) == k - 1), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_bins_table_and_image_equal_the_restatement(cb, name):
    hist = CASES[name]
    bins, lit, mx = cb.equalize_bins(hist)
    want_bins, want_lit, want_max = eq.bins(hist)
    assert (lit, mx) == (want_lit, want_max) == (int(np.count_nonzero(hist)), int(hist.max()))
    assert np.array_equal(bins, want_bins) and int(bins[0]) == 0
    for gamma in eq.GAMMAS:
        table, keys, levels = cb.equalize_table(bins, gamma)
        want_table, want_keys, want_levels = eq.table(cb, want_bins, gamma)
        assert (keys, levels) == (want_keys, want_levels) and np.array_equal(table, want_table), gamma
        gray, got_max, scale, got_lit = cb.set_grayscale_pixels_equalized(hist, gamma)
        want, _, _, _ = eq.image(cb, hist, gamma)
        assert gray.dtype == np.uint16 and gray.tobytes() == want.tobytes(), gamma
        # max and scale are the unflagged function's
        assert (got_max, got_lit) == (want_max, want_lit)
        assert scale == cb.set_grayscale_pixels(hist, gamma)[2]


@pytest.mark.parametrize("gamma", eq.GAMMAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_map_is_monotone_in_the_count(cb, name, gamma):
    hist = CASES[name].reshape(-1)
    gray = cb.set_grayscale_pixels_equalized(CASES[name], gamma)[0].reshape(-1)
    order = np.argsort(hist, kind="stable")
    assert np.all(np.diff(gray[order].astype(np.int64)) >= 0)
    assert not gray[hist == 0].any()
    if not hist.any():
        assert not gray.any()  # lit = 0: a zero image


@pytest.mark.parametrize("gamma", [g for g in eq.GAMMAS if g > 0])
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "all_zero"))
def test_the_brightest_lit_key_gets_65535(cb, name, gamma):
    """The brightest lit key has le = lit and gets 65535 -- also where cb_tone_value(lit, lit, gamma) does not give it:
    key_edges has lit = 162, and in doubles 162 * (65535.0 / 162) rounds to just under 65535, which gamma 1 and 0.5 keep
    there and the conversion truncates to 65534.  The definition pins that one entry of the table."""
    hist = CASES[name]
    gray = cb.set_grayscale_pixels_equalized(hist, gamma)[0]
    assert int(gray[hist == hist.max()].max()) == 65535


@pytest.mark.parametrize("gamma", eq.GAMMAS)
def test_distinct_counts_below_2048_get_their_rank(cb, gamma):
    hist = CASES["distinct_below_2048"]
    gray = cb.set_grayscale_pixels_equalized(hist, gamma)[0]
    lit = int(np.count_nonzero(hist))
    assert lit == 2047
    for c, v in zip(hist.reshape(-1).tolist(), gray.reshape(-1).tolist()):
        # the counters are 1 .. 2047, each once: the r-th smallest is r
        assert v == (cb.tone_value(c, lit, gamma) if c else 0), c


@pytest.mark.parametrize("name", ["distinct_below_2048", "heavy_tail", "colour_planes", "all_ones", "one_lit"])
def test_a_shift_of_every_counter_changes_nothing(cb, name):
    hist = CASES[name]
    room = 64 - int(hist.max()).bit_length()
    for gamma in (2.2, 0.0):
        want = cb.set_grayscale_pixels_equalized(hist, gamma)
        for j in sorted({1, 8, 11, room}):  # 8: the density filter's fraction bits; room: the largest that overflows nothing
            got = cb.set_grayscale_pixels_equalized(hist << np.uint64(j), gamma)
            assert got[0].tobytes() == want[0].tobytes() and got[3] == want[3], (gamma, j)
            assert got[1] == want[1] << j


def test_bad_arguments_are_refused_with_nothing_written(cb):
    hist = np.arange(12, dtype=np.uint64).reshape(3, 4)
    gray = np.zeros((3, 4), dtype=np.uint16)
    bins = np.full(eq.KEYS, 77, dtype=np.uint64)
    table = np.full(eq.KEYS, 77, dtype=np.uint16)
    out = [C.c_uint64(77) for _ in range(2)]
    refs = [C.byref(v) for v in out]
    f = cb.lib.cb_equalize_bins
    assert f(None, 12, bins.ctypes.data, *refs) == INVALID
    assert f(hist.ctypes.data, 0, bins.ctypes.data, *refs) == INVALID
    assert f(hist.ctypes.data, 12, None, *refs) == INVALID
    assert f(hist.ctypes.data, 12, bins.ctypes.data, None, refs[1]) == INVALID
    assert f(hist.ctypes.data, 12, bins.ctypes.data, refs[0], None) == INVALID
    good = np.zeros(eq.KEYS, dtype=np.uint64)
    good[5] = 3
    g = cb.lib.cb_equalize_table
    assert g(None, 1.0, table.ctypes.data, *refs) == INVALID
    assert g(good.ctypes.data, 1.0, None, *refs) == INVALID
    assert g(good.ctypes.data, 1.0, table.ctypes.data, None, refs[1]) == INVALID
    assert g(good.ctypes.data, 1.0, table.ctypes.data, refs[0], None) == INVALID
    e = cb.lib.cb_set_grayscale_pixels_equalized
    assert e(None, 4, 3, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert e(hist.ctypes.data, 4, 3, 1.0, None, None, None, None) == INVALID
    assert e(hist.ctypes.data, 0, 3, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert e(hist.ctypes.data, 4, -3, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert [v.value for v in out] == [77, 77] and not gray.any()
    assert set(bins.tolist()) == {77} and set(table.tolist()) == {77}
    # the three outputs of the image call are optional
    assert e(hist.ctypes.data, 4, 3, 1.0, gray.ctypes.data, None, None, None) == 0 and gray.any()
    assert f(hist.ctypes.data, 12, bins.ctypes.data, *refs) == 0 and [v.value for v in out] == [11, 11]
    assert g(good.ctypes.data, 1.0, table.ctypes.data, *refs) == 0 and [v.value for v in out] == [1, 1]
