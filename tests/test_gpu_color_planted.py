"""The colour stage on the device (color.hip) on planted planes (tests/output_planted.py): levels on bucket ends, on
exact cumulative boundaries, inside ties, in one bucket and behind the first sweep of the level kernels; stretched
values on every decision of color_math.h; outputs that are not 16-byte aligned.  A plane that holds one 65535 is its
own tone map at gamma 0, so the grey values are planted directly.  Byte for byte against cb_compose_color AND the numpy
restatement, with guard words around every output.  tests/test_output_planted_host.py shows that the plants are decisive."""

import functools

import numpy as np
import pytest

import color_reference as ref
import output_planted as op
from output_planted import guarded_output, on_device, read_guarded

pytestmark = pytest.mark.gpu

MODES = ("CB_TONE_LUT", "CB_TONE_THRESHOLDS")


def test_the_grid_named_here_is_the_code_s():
    text, said = op.source("color.hip")
    assert said == {"kColorThreads": op.COLOR_THREADS, "kLevelBlocksPerPlane": op.LEVEL_BLOCKS, "kComposeBlocks": op.COMPOSE_BLOCKS}
    assert (op.COLOR_THREADS, op.LEVEL_BLOCKS, op.COMPOSE_BLOCKS) == (256, 1024, 4096)
    assert "plane + g * 8ull" in text                          # eight pixels per lane
    assert op.LEVEL_SWEEP == 1024 * 256 * 8


def device_compose(cb, case, mode, compose, hue, offset=0):
    """The planes of a plant through cb_compose_color_device at gamma 0, the output GUARD + offset u16 into an allocation
    filled with FILL -> (big-endian samples [h, w, 3], levels), after the guards were seen untouched."""
    import torch

    h, w = case["planes"][0].shape
    samples = 3 * h * w
    held = [on_device(p) for p in case["planes"]]
    base, d_rgb = guarded_output(samples, offset)
    assert d_rgb.data_ptr() % 16 == (2 * offset) % 16
    levels = cb.compose_color_device([view.data_ptr() for _, view in held], w, h, 0.0, d_rgb.data_ptr(), mode=mode,
                                     compose=compose, stretch=case["stretch"], hue_shift=hue,
                                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return read_guarded(base, samples, offset).reshape(h, w, 3), levels


@functools.lru_cache(maxsize=None)
def plant(name):
    if name == "past_the_sweep":
        case = op.levels_past_the_sweep(op.LEVEL_SWEEP)
    elif name == "decisions":
        case = op.compose_decisions()
    else:
        case = op.level_case(name)
    for p in case["planes"]:
        p.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def references(cb, name, compose, hue):
    """Both host references of a plant, computed once -> (bytes of the image, levels)."""
    case = plant(name)
    grays = [p.astype(np.uint16) for p in case["planes"]]
    b, w = case["stretch"]
    want, want_levels = cb.compose_color(grays, compose=compose, stretch=(b, w), hue_shift=hue)
    np_rgb, np_levels = ref.compose(grays, compose, b, w, hue)
    assert want_levels == np_levels == [tuple(lv) for lv in case["levels"]]
    assert want.tobytes() == np_rgb.astype(">u2").tobytes()
    return want.tobytes(), want_levels


def check(cb, name, mode, compose, hue, offset=0):
    want, want_levels = references(cb, name, compose, hue)
    rgb, levels = device_compose(cb, plant(name), getattr(cb, mode), compose, hue, offset)
    assert levels == want_levels, (levels, want_levels)
    got = rgb.tobytes()
    if got != want:
        bad = np.flatnonzero(np.frombuffer(got, dtype=">u2") != np.frombuffer(want, dtype=">u2"))
        raise AssertionError("%d samples differ, the first at %s" % (bad.size, bad[:8]))
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(op.LEVEL_CASES))
def test_levels_on_planted_ranks(cb, name, mode):
    """Item 6: the two-pass select returns the designed levels -- a positive black in eleven planes of twelve -- and the image
    stretched by them is the references'."""
    check(cb, name, mode, "rgb", 0.0)
    check(cb, name, mode, "hsl", 0.3)


@pytest.mark.parametrize("mode", MODES)
def test_levels_decided_past_the_first_sweep(cb, mode):
    """Item 7: the eleven pixels that decide both levels are read by the second trip of the level kernels' loops."""
    case = plant("past_the_sweep")
    assert case["planes"][0].size == op.LEVEL_SWEEP + 11
    check(cb, "past_the_sweep", mode, "rgb", 0.0)


@pytest.mark.parametrize("compose,hue", op.COMPOSES)
@pytest.mark.parametrize("mode", MODES)
def test_compose_decisions(cb, mode, compose, hue):
    """Item 8: s of 0 and 1, L around 0.5 and hues around 1/6, 1/2 and 2/3 in every combination."""
    check(cb, "decisions", mode, compose, hue)


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("mode", MODES)
def test_output_alignment(cb, mode, offset):
    """Item 9: an output 2 and 8 bytes off a 16-byte boundary takes the per-sample stores for every group; the bytes are
    those of the aligned run."""
    for compose, hue in op.COMPOSES:
        aligned = check(cb, "decisions", mode, compose, hue)
        assert check(cb, "decisions", mode, compose, hue, offset) == aligned, (compose, hue)
