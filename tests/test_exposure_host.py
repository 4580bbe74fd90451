"""The white clip on the host (include/cudabrot_amd.h, "White clip"), without a GPU: cb_white_count and
cb_set_grayscale_pixels_white against the numpy restatement of the definition (tests/exposure_reference.py), the invariants
of the definition asserted directly, the p = 0 anchor against cb_set_grayscale_pixels, and the refusals."""

import ctypes as C

import numpy as np
import pytest

import exposure_reference as expo

INVALID = 1  # hipErrorInvalidValue
CASES = expo.cases()


def clips_of(name):
    return expo.CLIPS + (expo.BOUNDARY_CLIPS if name == "rank_on_a_boundary" else ())


@pytest.mark.parametrize("name", sorted(CASES))
def test_white_count_equals_the_restatement_and_keeps_the_invariants(cb, name):
    hist = CASES[name]
    flat = hist.reshape(-1)
    for clip in clips_of(name):
        white, lit, clipped = cb.white_count(hist, clip)
        assert (white, lit, clipped) == expo.white_count(hist, clip), clip
        assert lit == int(np.count_nonzero(flat))
        r = expo.rank(lit, clip)
        assert cb.lib.cb_white_rank(lit, clip) == r
        assert clipped == int(np.count_nonzero(flat > np.uint64(white))) <= r
        if lit:
            assert int(np.count_nonzero(flat >= np.uint64(white))) > r and white > 0
        else:
            assert white == 0 and clipped == 0


def test_the_anchors_of_the_definition(cb):
    for name, hist in CASES.items():
        lit = hist[hist > 0]
        assert cb.white_count(hist, 0.0)[0] == int(hist.max()), name          # p = 0: the maximum
        smallest = int(lit.min()) if lit.size else 0
        assert cb.white_count(hist, 99.999999)[0] == smallest, name           # p just under 100: the smallest lit counter
    # one repeated value: every rank lands inside the one run of ties
    assert {cb.white_count(CASES["one_repeated_value"], p) for p in expo.CLIPS} == {(42, 17 * 19, 0)}
    # the rank exactly between two distinct values, from both sides
    b = CASES["rank_on_a_boundary"]
    assert [expo.rank(1000, p) for p in expo.BOUNDARY_CLIPS] == [9, 10]
    assert cb.white_count(b, 0.9) == (900, 1000, 0) and cb.white_count(b, 1.0) == (7, 1000, 10)
    # every planted counter beyond 32 bits is a white point of its own
    hot = CASES["beyond_32_bits"]
    n_lit = int(np.count_nonzero(hot))
    top = sorted((int(v) for v in hot.reshape(-1)), reverse=True)[:5]
    assert top[:4] == [(1 << 63) + 1, 1 << 56, (1 << 37) + 12345, 1 << 32]
    for k in range(5):
        assert cb.white_count(hot, 100.0 * (k + 0.5) / n_lit) == (top[k], n_lit, k)


@pytest.mark.parametrize("gamma", expo.GAMMAS)
def test_clip_zero_is_set_grayscale_pixels(cb, gamma):
    for name, hist in CASES.items():
        gray, mx, scale, white = cb.set_grayscale_pixels_white(hist, gamma, 0.0)
        want, want_max, want_scale = cb.set_grayscale_pixels(hist, gamma)
        assert (mx, white) == (want_max, want_max) and scale == want_scale, name
        assert gray.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("gamma", expo.GAMMAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_clipped_image_equals_the_restatement(cb, name, gamma):
    hist = CASES[name]
    for clip in (0.1, 1.0, 50.0, 99.0) + (expo.BOUNDARY_CLIPS if name == "rank_on_a_boundary" else ()):
        gray, mx, scale, white = cb.set_grayscale_pixels_white(hist, gamma, clip)
        want, want_white = expo.tone_map(cb, hist, gamma, clip)
        assert white == want_white and mx == int(hist.max())                   # max stays the true maximum
        assert scale == (65535.0 / white if white else float("inf"))          # ... and scale is the one applied
        assert gray.dtype == np.uint16 and gray.tobytes() == want.tobytes()
        above = hist > np.uint64(white)
        if above.any():                                                        # what lies above white has white's value
            assert set(gray[above].tolist()) == {cb.tone_value(white, white, gamma)}


def test_bad_arguments_are_refused(cb):
    hist = np.arange(12, dtype=np.uint64).reshape(3, 4)
    gray = np.zeros((3, 4), dtype=np.uint16)
    out = [C.c_uint64(77) for _ in range(3)]
    refs = [C.byref(v) for v in out]
    for bad in (-1.0, -1e-300, 100.0, 1e9, float("nan"), float("inf"), float("-inf")):
        assert cb.lib.cb_white_clip_ok(bad) == 0
        assert cb.lib.cb_white_count(hist.ctypes.data, 12, bad, *refs) == INVALID
        assert cb.lib.cb_set_grayscale_pixels_white(hist.ctypes.data, 4, 3, 1.0, bad, gray.ctypes.data, None, None, None) == INVALID
        with pytest.raises(cb.CudabrotError):
            cb.white_count(hist, bad)
    for good in (0.0, 0.1, 99.999999, float.fromhex("0x1.8p+6") - 1.0):
        assert cb.lib.cb_white_clip_ok(good) == 1
    assert cb.lib.cb_white_count(None, 12, 1.0, *refs) == INVALID
    for k in range(3):
        holed = list(refs)
        holed[k] = None
        assert cb.lib.cb_white_count(hist.ctypes.data, 12, 1.0, *holed) == INVALID
    assert cb.lib.cb_set_grayscale_pixels_white(None, 4, 3, 1.0, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert cb.lib.cb_set_grayscale_pixels_white(hist.ctypes.data, 4, 3, 1.0, 1.0, None, None, None, None) == INVALID
    assert cb.lib.cb_set_grayscale_pixels_white(hist.ctypes.data, 0, 3, 1.0, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert cb.lib.cb_set_grayscale_pixels_white(hist.ctypes.data, 4, -3, 1.0, 1.0, gray.ctypes.data, None, None, None) == INVALID
    assert [v.value for v in out] == [77, 77, 77] and not gray.any()            # a refusal writes nothing
    # the three outputs of the image call are optional, and an empty array is an array
    assert cb.lib.cb_set_grayscale_pixels_white(hist.ctypes.data, 4, 3, 1.0, 50.0, gray.ctypes.data, None, None, None) == 0
    assert cb.lib.cb_white_count(hist.ctypes.data, 0, 1.0, *refs) == 0 and [v.value for v in out] == [0, 0, 0]
