"""The locally equalised image on the host (include/cudabrot_amd.h, "Locally equalised image"), without a
GPU: cb_local_equalize_bins, cb_local_equalize_clip and cb_set_grayscale_pixels_local_equalized against the restatement in
Python integers (tests/local_equalize_reference.py) on every shared case and every grid that fits it, the consequences the
definition states asserted directly, the clip at its edges, and the refusals."""

import ctypes as C

import numpy as np
import pytest

import equalize_reference as eq
import local_equalize_reference as leq

INVALID = 1  # hipErrorInvalidValue
CASES = leq.cases()
FITTING = [(name, grid) for name in sorted(CASES) for grid in leq.GRIDS if leq.fits(CASES[name], grid)]


def sparse(dense):
    return {int(k): int(dense[k]) for k in np.flatnonzero(dense)}


def test_the_constants_are_the_header_s(cb):
    assert cb.CB_LOCAL_EQUALIZE_MAX_TILES == 16 == max(max(g) for g in leq.GRIDS)
    assert cb.LOCAL_EQUALIZE_CLIP_Q == 1024 in leq.CLIPS
    assert {name for name, _ in FITTING} == set(CASES)


@pytest.mark.parametrize("name,grid", FITTING)
def test_bins_and_image_equal_the_restatement(cb, name, grid):
    hist, (tx, ty) = CASES[name], grid
    bins, lit, mx = cb.local_equalize_bins(hist, tx, ty)
    want_bins = leq.tile_bins(hist, tx, ty)
    assert bins.shape == (tx * ty, eq.KEYS) and np.array_equal(bins, leq.dense(want_bins))
    assert (lit, mx) == (int(np.count_nonzero(hist)), int(np.max(hist)))
    for clip_q in leq.CLIPS:
        for gamma in leq.GAMMAS if clip_q == 1024 else leq.GAMMAS[:1]:
            gray, got_max, scale, *numbers = cb.set_grayscale_pixels_local_equalized(hist, tx, ty, clip_q, gamma)
            want, *want_numbers = leq.image(cb, hist, tx, ty, clip_q, gamma)
            assert gray.dtype == np.uint16 and gray.shape == hist.shape
            assert gray.tobytes() == want.tobytes(), (clip_q, gamma, np.argwhere(gray != want)[:4])
            assert numbers == want_numbers and numbers[0] == lit and numbers[1] == sum(1 for b in want_bins if b)
            # max and scale are the unflagged function's over the whole array
            assert got_max == mx and scale == cb.set_grayscale_pixels(hist.reshape(-1, hist.shape[-1]), gamma)[2]
            assert not gray[hist == 0].any()


@pytest.mark.parametrize("gamma", eq.GAMMAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_tile_without_a_clip_is_the_equalised_image(cb, name, gamma):
    hist = CASES[name]
    rows = hist.reshape(-1, hist.shape[-1])  # planes pooled: one table over all of them
    planes = hist.shape[0] if hist.ndim == 3 else 1
    got = cb.set_grayscale_pixels_local_equalized(hist, 1, 1, 0, gamma)
    want = cb.set_grayscale_pixels_equalized(rows, gamma)
    assert got[0].tobytes() == want[0].tobytes() and got[1:4] == want[1:]
    assert got[4:] == (1 if want[3] else 0, 0) and planes in (1, 3)


@pytest.mark.parametrize("clip_q", leq.CLIPS)
@pytest.mark.parametrize("grid", [(1, 1), (3, 2), (8, 8)])
def test_the_value_is_monotone_in_the_count_at_a_fixed_position(cb, grid, clip_q):
    """The planes of an image share the tiles' tables: the twelve counters that stand at one position in twelve planes are
    mapped by one blend of four monotone tables."""
    rng = np.random.default_rng(3)
    hist = eq.heavy(rng, 12 * 16 * 24, 1 << 30).reshape(12, 16, 24)
    for gamma in leq.GAMMAS:
        gray = cb.set_grayscale_pixels_local_equalized(hist, *grid, clip_q, gamma)[0]
        order = np.argsort(hist, axis=0, kind="stable")
        assert np.all(np.diff(np.take_along_axis(gray, order, axis=0).astype(np.int64), axis=0) >= 0)
        assert np.array_equal(np.sort(gray, axis=0), np.take_along_axis(gray, order, axis=0))


@pytest.mark.parametrize("grid", [(2, 2), (4, 3), (16, 16)])
def test_identical_tiles_give_each_tile_its_own_equalised_image(cb, grid):
    tx, ty = grid
    tile = eq.heavy(np.random.default_rng(11), 5 * 7, 1 << 22).reshape(5, 7) + np.uint64(1)
    hist = np.tile(tile, (ty, tx))
    for gamma in leq.GAMMAS:
        own = cb.set_grayscale_pixels_equalized(tile, gamma)[0]
        got = cb.set_grayscale_pixels_local_equalized(hist, tx, ty, 0, gamma)
        assert np.array_equal(got[0], np.tile(own, (ty, tx))) and got[4] == tx * ty


def test_a_pixel_at_a_tile_centre_takes_that_tile_s_table_alone(cb):
    """15 x 9 in 3 x 3 tiles of 5 x 3: 2x + 1 = CX[i] at x = 2, 7, 12 and 2y + 1 = CY[j] at y = 1, 4, 7."""
    hist = eq.heavy(np.random.default_rng(17), 9 * 15, 1 << 30).reshape(9, 15) + np.uint64(1)
    assert leq.centres(15, 3) == [5, 15, 25] and leq.centres(9, 3) == [3, 9, 15]
    for gamma in leq.GAMMAS:
        gray = cb.set_grayscale_pixels_local_equalized(hist, 3, 3, 0, gamma)[0]
        elsewhere = 0
        for j in range(3):
            for i in range(3):
                own = cb.set_grayscale_pixels_equalized(hist[3 * j:3 * j + 3, 5 * i:5 * i + 5], gamma)[0]
                assert gray[3 * j + 1, 5 * i + 2] == own[1, 2], (i, j)
                elsewhere += int(np.count_nonzero(gray[3 * j:3 * j + 3, 5 * i:5 * i + 5] != own))
        assert elsewhere > 0  # the other pixels are blends


@pytest.mark.parametrize("name", ["heavy_odd", "three_planes", "crowded", "all_ones", "one_lit"])
def test_a_shift_of_every_counter_changes_nothing(cb, name):
    hist = CASES[name]
    grid = (4, 3) if leq.fits(hist, (4, 3)) else (2, 2)
    room = 64 - int(hist.max()).bit_length()
    for clip_q, gamma in ((1024, 2.2), (0, 0.0)):
        want = cb.set_grayscale_pixels_local_equalized(hist, *grid, clip_q, gamma)
        for s in sorted({1, 8, room}):  # 8: the density filter's fraction bits; room: the largest that overflows nothing
            got = cb.set_grayscale_pixels_local_equalized(hist << np.uint64(s), *grid, clip_q, gamma)
            assert got[0].tobytes() == want[0].tobytes() and got[3:] == want[3:] and got[1] == want[1] << s, (clip_q, s)


def dense_of(b):
    out = np.zeros(eq.KEYS, dtype=np.uint64)
    for k, n in b.items():
        out[k] = n
    return out


@pytest.mark.parametrize(
    "b,clip_q,want,moved",
    [({1: 11, 2: 1, 3: 1}, 256, {1: 7, 2: 3, 3: 3}, 7),              # L = 4, E = 7: 7 mod 3 = 1 goes to the first lit key
     ({1: 3, 2: 1, 3: 1}, 256, {1: 2, 2: 2, 3: 1}, 2),              # floor(5 / 3) = 1: the limit is floored to 1
     ({4000: 1 << 39}, 256, {4000: 1 << 39}, 0),                    # one lit key: nothing to clip
     ({7: 100, 56319: 1}, 512, {7: 100, 56319: 1}, 0),              # L = 101
     ({7: 100, 56319: 1}, 256, {7: 75, 56319: 26}, 50),             # L = 50: E = 50, 25 each
     ({1: 11, 2: 1, 3: 1}, 0, {1: 11, 2: 1, 3: 1}, 0),              # off
     ({k: (1 << 40) // 5 for k in range(1, 6)}, 65536, {k: (1 << 40) // 5 for k in range(1, 6)}, 0)],  # clip_q * lit < 2^57
)
def test_the_clip_at_its_edges(cb, b, clip_q, want, moved):
    assert leq.clip(b, clip_q) == (want, moved)
    clipped, got_moved = cb.local_equalize_clip(dense_of(b), clip_q)
    assert sparse(clipped) == want and got_moved == moved
    assert int(clipped.sum()) == sum(b.values()) and set(np.flatnonzero(clipped).tolist()) == set(b)


@pytest.mark.parametrize("name,grid", [("crowded", (4, 3)), ("heavy_odd", (5, 3)), ("empty_half", (4, 3)), ("all_ones", (2, 2))])
def test_clipped_bins_keep_every_tile_s_lit_and_its_lit_keys(cb, name, grid):
    bins = cb.local_equalize_bins(CASES[name], *grid)[0]
    total = 0
    for clip_q in (256, 1024, 65536):
        for t in range(bins.shape[0]):
            clipped, moved = cb.local_equalize_clip(bins[t], clip_q)
            assert int(clipped.sum()) == int(bins[t].sum()) and np.array_equal(clipped != 0, bins[t] != 0), (clip_q, t)
            assert (sparse(clipped), moved) == leq.clip(sparse(bins[t]), clip_q)
            total += moved
    assert total > 0 or name == "all_ones"  # a tile with one lit key has nothing to clip


def test_an_empty_tile_beside_a_lit_one_takes_the_global_table(cb):
    """Two tiles, the right one empty: its table is the global one, which is the left tile's -- so without a clip the image
    is the equalised image, and the lit pixels right of the left centre are not pulled towards black."""
    hist = np.zeros((6, 20), dtype=np.uint64)
    hist[:, :10] = eq.heavy(np.random.default_rng(23), 60, 1 << 20).reshape(6, 10) + np.uint64(1)
    for gamma in leq.GAMMAS:
        got = cb.set_grayscale_pixels_local_equalized(hist, 2, 1, 0, gamma)
        assert got[0].tobytes() == cb.set_grayscale_pixels_equalized(hist, gamma)[0].tobytes()
        assert got[3:] == (60, 1, 0) and got[0][:, 5:10].all()
    # three tiles, the middle one empty, takes the table of both lit ones together
    hist = np.zeros((4, 30), dtype=np.uint64)
    hist[:, :10] = np.arange(1, 41, dtype=np.uint64).reshape(4, 10)
    hist[:, 20:] = np.arange(1001, 1041, dtype=np.uint64).reshape(4, 10)
    got = cb.set_grayscale_pixels_local_equalized(hist, 3, 1, 0, 1.0)
    want = leq.image(cb, hist, 3, 1, 0, 1.0)
    assert got[0].tobytes() == want[0].tobytes() and got[3:] == tuple(want[1:]) == (80, 2, 0)
    # x = 9: 9/20 of the way from the left centre to the middle one; the largest count of the left tile is full white in its
    # own table and half of it in the global one
    assert int(hist[3, 9]) == 40 and int(got[0][3, 9]) == (11 * 65535 + 9 * cb.tone_value(40, 80, 1.0) + 10) // 20


def test_bad_arguments_are_refused_with_nothing_written(cb):
    hist = np.arange(1, 25, dtype=np.uint64).reshape(2, 3, 4)
    gray = np.zeros((2, 3, 4), dtype=np.uint16)
    bins = np.full((4, eq.KEYS), 77, dtype=np.uint64)
    out = [C.c_uint64(77) for _ in range(3)]
    refs = [C.byref(v) for v in out]
    p, g, b = hist.ctypes.data, gray.ctypes.data, bins.ctypes.data
    bad_grids = [(4, 3, 2, 0, 1), (4, 3, 2, 1, 0), (4, 3, 2, 5, 1), (4, 3, 2, 1, 4), (4, 3, 2, 17, 1), (4, 3, 2, -1, 1),
                 (0, 3, 2, 1, 1), (4, 0, 2, 1, 1), (-4, 3, 2, 1, 1), (4, 3, 0, 1, 1), (4, 3, -1, 1, 1)]
    f = cb.lib.cb_local_equalize_bins
    for call in [(None, 4, 3, 2, 2, 2, b, *refs[:2]), (p, 4, 3, 2, 2, 2, None, *refs[:2]), (p, 4, 3, 2, 2, 2, b, None, refs[1]),
                 (p, 4, 3, 2, 2, 2, b, refs[0], None)] + [(p, *grid, b, *refs[:2]) for grid in bad_grids]:
        assert f(*call) == INVALID, call
    e = cb.lib.cb_set_grayscale_pixels_local_equalized
    for call in ([(None, 4, 3, 2, 2, 2, 1024, 1.0, g), (p, 4, 3, 2, 2, 2, 1024, 1.0, None)]
                 + [(p, *grid, 1024, 1.0, g) for grid in bad_grids]
                 + [(p, 4, 3, 2, 2, 2, clip_q, 1.0, g) for clip_q in (1, 255, 65537, 1 << 31)]):
        assert e(*call, None, None, *refs) == INVALID, call
    c = cb.lib.cb_local_equalize_clip
    moved = C.c_uint64(77)
    good = np.zeros(eq.KEYS, dtype=np.uint64)
    good[5] = 3
    for call in [(None, 256, b), (good.ctypes.data, 256, None), (good.ctypes.data, 255, b), (good.ctypes.data, 65537, b)]:
        assert c(*call, C.byref(moved)) == INVALID, call
    assert c(good.ctypes.data, 256, b, None) == INVALID
    assert [v.value for v in out] == [77, 77, 77] and moved.value == 77 and not gray.any() and set(bins.reshape(-1).tolist()) == {77}
    assert [cb.lib.cb_local_equalize_ok(4, 3, 2, 4, 3, q) for q in (0, 255, 256, 65536, 65537)] == [1, 0, 1, 1, 0]
    # every output number of the image call is optional
    assert e(p, 4, 3, 2, 2, 2, 1024, 1.0, g, None, None, None, None, None) == 0 and gray.all()
    assert f(p, 4, 3, 2, 2, 2, b, *refs[:2]) == 0 and [v.value for v in out[:2]] == [24, 24] and int(bins.sum()) == 24
    assert c(good.ctypes.data, 256, b, C.byref(moved)) == 0 and moved.value == 0 and int(bins[0].sum()) == 3
