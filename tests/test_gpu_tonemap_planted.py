"""The device tone map (tonemap.hip) on planted histograms (tests/output_planted.py): every count of a domain, both
sides of every threshold beyond the table's reach, counters decided behind the first sweep of the grid, one to three
pixels, and the clamped table of the white clip.  Byte for byte against the host functions, with guard words around
every output.  tests/test_output_planted_host.py shows that the plants are decisive."""

import functools
import re

import numpy as np
import pytest

import output_planted as op
from output_planted import guarded_output, on_device, read_guarded

pytestmark = pytest.mark.gpu

MODES = ("CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO")


def test_the_grid_named_here_is_the_code_s():
    text, said = op.source("counter_sweep.h")  # the lookup loop, its lanes and its grid are the header's
    assert said["kSweepThreads"] == op.TONE_THREADS == 256
    caps = re.findall(r"if \(blocks > (\d+)ull \* (\d+)ull\) blocks = (\d+)ull \* (\d+)ull;", text)
    assert len(caps) == 1 and int(caps[0][0]) * int(caps[0][1]) == int(caps[0][2]) * int(caps[0][3]) == op.TONE_BLOCK_CAP
    assert text.count("* kSweepThreads * 2ull") == 1           # two pixels per lane, in the one loop: map_pairs
    assert op.source("tonemap.hip")[0].count("map_pairs(hist, n, out_be,") == 2  # the table's and the thresholds' kernel
    assert op.TONE_SWEEP == 2 * 4096 * 256


def device_tone(cb, hist, gamma, mode, clip=None):
    """hist as one row through cb_tone_map_device (or ..._white) -> (values, max, scale, white)."""
    import torch

    n = hist.size
    keep, d_hist = on_device(hist)
    base, d_gray = guarded_output(n)
    assert d_gray.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    try:
        if clip is None:
            mx, scale = cb.tone_map_device(d_hist.data_ptr(), n, 1, gamma, d_gray.data_ptr(), mode=mode, stream=stream)
            white = mx
        else:
            mx, scale, white = cb.tone_map_device_white(d_hist.data_ptr(), n, 1, gamma, clip, d_gray.data_ptr(), mode=mode,
                                                        stream=stream)
    finally:
        torch.cuda.synchronize()
        body = read_guarded(base, n)  # the guards hold for a refused call too
    return body.astype(np.uint16), mx, scale, white


def same_image(got, want):
    assert got.shape == want.reshape(-1).shape
    assert got.tobytes() == want.reshape(-1).tobytes(), np.flatnonzero(got != want.reshape(-1))[:8]


@functools.lru_cache(maxsize=None)
def domain(top):
    a = op.every_count(top)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_image(cb, kind, top, gamma):
    """The host's image of a plant, computed once -> (plant, host values, max, scale)."""
    if kind == "domain":
        hist = domain(top)
    elif kind == "beyond":
        hist = op.beyond_the_table(op.host_map(cb, top, gamma), top)[0]
    else:
        hist = op.past_the_first_sweep(op.host_map(cb, top, gamma), op.TONE_SWEEP, top)[0]
    gray, mx, scale = cb.set_grayscale_pixels(hist.reshape(1, -1), gamma)
    for a in (hist, gray):
        a.setflags(write=False)
    return hist, gray, mx, scale


@pytest.mark.parametrize("gamma", op.GAMMAS)
@pytest.mark.parametrize("top", op.DOMAIN_TOPS)
def test_every_count_of_a_domain(cb, top, gamma):
    """Item 1: each count of [0, top] is a pixel, so every entry of the table is read and every threshold has the count
    on it and the count below it."""
    hist, gray, want_max, want_scale = host_image(cb, "domain", top, gamma)
    if (top, gamma) == (162, 1.0):
        assert int(gray.max()) == 65534  # the last threshold has no count
    for mode in ("CB_TONE_LUT", "CB_TONE_THRESHOLDS"):
        body, mx, scale, _ = device_tone(cb, hist, gamma, getattr(cb, mode))
        assert (mx, scale) == (want_max, want_scale) and mx == top, mode
        same_image(body, gray)


@pytest.mark.parametrize("gamma", op.GAMMAS)
@pytest.mark.parametrize("top", op.BEYOND_TOPS)
def test_both_sides_of_every_threshold_beyond_the_table(cb, top, gamma):
    """Item 2: t - 1 and t for the smallest count t that reaches each output value, under maxima up to 2^64 - 1."""
    hist, gray, want_max, want_scale = host_image(cb, "beyond", top, gamma)
    assert hist.size % 2 == 1 and want_max == top
    for mode in ("CB_TONE_AUTO", "CB_TONE_THRESHOLDS"):
        body, mx, scale, _ = device_tone(cb, hist, gamma, getattr(cb, mode))
        assert mx == top and scale == want_scale, mode
        same_image(body, gray)
    if top >= 1 << 32:
        with pytest.raises(cb.CudabrotError):  # no table of 2^32 entries or more; the guards are checked on this path too
            device_tone(cb, hist, gamma, cb.CB_TONE_LUT)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("top", [1 << 40, (1 << 24) - 1])
def test_counters_past_the_first_sweep(cb, top, mode):
    """Item 3: one full sweep of the capped grid and three counters more; the maximum is the last of them.  Under 2^40
    the table is refused, so the same array under 2^24 - 1, the largest maximum AUTO gives a table, takes the table
    kernel round its loop a second time."""
    hist, gray, want_max, want_scale = host_image(cb, "sweep", top, 2.2)
    assert hist.size == op.TONE_SWEEP + 3 and want_max == top
    if mode == "CB_TONE_LUT" and top >= 1 << 32:
        with pytest.raises(cb.CudabrotError):
            device_tone(cb, hist, 2.2, cb.CB_TONE_LUT)
        return
    body, mx, scale, _ = device_tone(cb, hist, 2.2, getattr(cb, mode))
    assert (mx, scale) == (top, want_scale)
    same_image(body, gray)
    assert body[-3] == 0 and 0 < body[-2] < body[-1] == gray.max()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_and_odd(cb, n):
    """Item 4: one lone store, one paired store, one of each."""
    hist = op.tiny(n)
    for gamma in op.GAMMAS:
        gray, want_max, want_scale = cb.set_grayscale_pixels(hist.reshape(1, -1), gamma)
        for mode in MODES:
            body, mx, scale, _ = device_tone(cb, hist, gamma, getattr(cb, mode))
            assert (mx, scale) == (want_max, want_scale) == (5, 65535.0 / 5.0), (gamma, mode)
            same_image(body, gray)


@pytest.mark.parametrize("gamma", op.GAMMAS)
def test_the_clamp_instance(cb, gamma):
    """Item 5: every count of [0, 1 000 003] under a 50 % clip: the white point falls below the maximum, the table ends
    there and about half of the counters lie above it."""
    hist = domain(1_000_003)
    gray, want_max, want_scale, want_white = cb.set_grayscale_pixels_white(hist.reshape(1, -1), gamma, 50.0)
    assert want_white < want_max == 1_000_003 and np.count_nonzero(hist > np.uint64(want_white)) > 400_000
    for mode in MODES:
        body, mx, scale, white = device_tone(cb, hist, gamma, getattr(cb, mode), clip=50.0)
        assert (mx, scale, white) == (want_max, want_scale, want_white), mode
        same_image(body, gray)
