"""The colour stage on the host (include/cudabrot_amd.h, "Colour image"): cb_compose_color against the numpy float64
restatement of the definition (tests/color_reference.py), byte for byte and levels included; the PPM writer; every
rejected parameter; the CLI's colour flags where they fail before any device work."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import color_reference as ref


def _planes(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "skewed":                       # a Buddhabrot plane: 90 % zeros, a heavy tail
        g = np.minimum(rng.pareto(1.0, size=(h, w)) * 900.0, 65535).astype(np.uint16)
        g[rng.random((h, w)) < 0.9] = 0
        return g
    if kind == "uniform":
        return rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    if kind == "zero":
        return np.zeros((h, w), dtype=np.uint16)
    if kind == "constant":
        return np.full((h, w), 40000, dtype=np.uint16)
    raise ValueError(kind)


def _check(cb, grays, compose, stretch, hue):
    rgb, levels = cb.compose_color(grays, compose=compose, stretch=stretch, hue_shift=hue)
    want, want_levels = ref.compose(grays, compose, stretch[0], stretch[1], hue)
    assert levels == want_levels
    assert rgb.dtype == np.dtype(">u2") and rgb.shape == want.shape
    assert rgb.tobytes() == want.astype(">u2").tobytes()
    return levels


@pytest.mark.parametrize("compose", ["rgb", "hsl"])
@pytest.mark.parametrize("h,w", [(1, 1), (77, 333), (768, 1024)])
@pytest.mark.parametrize("kinds", [("skewed", "skewed", "skewed"), ("uniform", "uniform", "uniform"),
                                   ("skewed", "zero", "constant")], ids=["skewed", "uniform", "zero_constant"])
@pytest.mark.parametrize("stretch,hue", [((2.0, 1.0), 0.0), ((0.0, 0.0), -1.7), ((2.0, 1.0), 0.3), ((5.0, 10.0), 2.0)])
def test_host_compose_equals_numpy_restatement(cb, compose, h, w, kinds, stretch, hue):
    grays = [_planes(k, h, w, 17 * j + h) for j, k in enumerate(kinds)]
    _check(cb, grays, compose, stretch, hue)


def test_flat_planes_have_white_at_or_below_black(cb):
    """white <= black (an all-zero or constant plane): every pixel at the black level is 0, the rest 1."""
    grays = [_planes("zero", 33, 21, 0), _planes("constant", 33, 21, 0), _planes("skewed", 33, 21, 5)]
    levels = _check(cb, grays, "rgb", (2.0, 1.0), 0.0)
    assert levels[0] == (0, 0) and levels[1] == (40000, 40000)
    rgb, _ = cb.compose_color(grays, "rgb")
    assert not rgb[..., 0].any() and not rgb[..., 1].any()


def test_levels_are_the_normalize_percentiles(cb):
    """1000 distinct values, 2 % / 1 %: black is the 21st smallest, white the 11th largest."""
    v = np.random.default_rng(3).permutation(np.arange(1000, dtype=np.uint16) * 60).reshape(40, 25)
    _, levels = cb.compose_color([v, v, v], "rgb", stretch=(2.0, 1.0))
    assert levels == [(20 * 60, 989 * 60)] * 3
    _, levels = cb.compose_color([v, v, v], "rgb", stretch=(0.0, 0.0))
    assert levels == [(0, 999 * 60)] * 3


def test_hsl_of_grey_and_of_pure_hues(cb):
    """S = 0 gives grey (R = G = B = L); full S at L = 0.5 gives the primaries at hue 0, 1/3, 2/3."""
    ramp = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    zero = np.zeros_like(ramp)
    rgb, _ = cb.compose_color([ramp, zero, ramp], "hsl", stretch=(0.0, 0.0))
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    assert np.array_equal(rgb[..., 0].astype(np.uint16), ramp)


def test_save_ppm_header_and_body(cb, tmp_path):
    grays = [_planes(k, 7, 5, 9) for k in ("uniform", "skewed", "uniform")]
    rgb, _ = cb.compose_color(grays, "hsl", hue_shift=0.3)
    path = str(tmp_path / "c.ppm")
    assert cb.save_ppm(path, rgb) == 0
    with open(path, "rb") as f:
        data = f.read()
    assert data.startswith(b"P6\n5 7\n65535\n")
    assert data == ref.ppm_bytes(ref.compose(grays, "hsl", 2.0, 1.0, 0.3)[0])
    assert len(data) == len(b"P6\n5 7\n65535\n") + 7 * 5 * 6
    assert cb.save_ppm(str(tmp_path / "missing" / "c.ppm"), rgb) == 1        # open failure, as cb_save_image


def test_every_bad_color_parameter_is_rejected(cb):
    lib = cb.capi.lib
    g = np.zeros(12, dtype=np.uint16)
    ptrs = (C.c_void_p * 3)(g.ctypes.data, g.ctypes.data, g.ctypes.data)
    out = np.zeros(36, dtype=np.uint16)
    lev = np.zeros(6, dtype=np.uint16)
    null = C.c_void_p(0)
    P = cb.ColorParams

    def host(p, ptrs=ptrs, w=3, h=4, out_ptr=out.ctypes.data):
        return lib.cb_compose_color(ptrs, w, h, C.byref(p) if p is not None else None, out_ptr, lev.ctypes.data)

    assert host(P(0, 2.0, 1.0, 0.0)) == 0 and host(P(1, 49.0, 50.0, -3.0)) == 0
    nan, inf = float("nan"), float("inf")
    bad_params = [P(2, 2.0, 1.0, 0.0), P(-1, 2.0, 1.0, 0.0), P(0, -0.5, 1.0, 0.0), P(0, 2.0, -1.0, 0.0),
                  P(0, 50.0, 50.0, 0.0), P(0, 99.5, 0.6, 0.0), P(0, nan, 1.0, 0.0), P(0, 2.0, inf, 0.0),
                  P(1, 2.0, 1.0, nan), P(1, 2.0, 1.0, -inf)]
    invalid = 1  # hipErrorInvalidValue
    for p in bad_params:
        assert host(p) == invalid, (p.compose, p.black_percent, p.white_percent, p.hue_shift)
    ok = P(0, 2.0, 1.0, 0.0)
    assert host(None) == invalid
    assert host(ok, ptrs=None) == invalid
    assert host(ok, ptrs=(C.c_void_p * 3)(g.ctypes.data, None, g.ctypes.data)) == invalid
    assert host(ok, out_ptr=None) == invalid
    assert host(ok, w=0) == invalid and host(ok, h=-1) == invalid
    # the device entry points refuse the same parameters before any device work
    for p in bad_params + [None]:
        ref_p = C.byref(p) if p is not None else None
        assert lib.cb_compose_color_device(ptrs, 3, 4, 1.0, 0, ref_p, out.ctypes.data, lev.ctypes.data, null) == invalid
    assert lib.cb_compose_color_device(None, 3, 4, 1.0, 0, C.byref(ok), out.ctypes.data, None, null) == invalid
    assert lib.cb_compose_color_device(ptrs, 3, 4, 1.0, 0, C.byref(ok), None, None, null) == invalid
    assert lib.cb_compose_color_device(ptrs, 0, 4, 1.0, 0, C.byref(ok), out.ctypes.data, None, null) == invalid
    idx = (C.c_int * 3)(0, 1, 2)
    assert lib.cb_renderer_color_image(null, idx, 1.0, 0, C.byref(ok), out.ctypes.data, None) == invalid
    assert lib.cb_save_ppm_be(None, out.ctypes.data, 3, 4) == 1
    with pytest.raises(ValueError):
        cb.compose_color([g.reshape(3, 4)] * 3, compose="cmyk")


# ---- the CLI: flags that fail before any device work (message, then usage, exit 0, like every bad argument) ----

@pytest.fixture(scope="module")
def exe(repo_root):
    path = os.path.join(repo_root, "cudabrot")
    if not os.access(path, os.X_OK):
        pytest.fail("./cudabrot is not built (run `make` or __graft_entry__.build())")
    return path


def run(exe, *args, **kw):
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, **kw)


CH3 = ["--channel", "100:20:a.pgm", "--channel", "400:100:b.pgm", "--channel", "1500:400:c.pgm"]


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
        (["--color", "c.ppm", *CH3[:4]], "--color needs exactly 3 --channel images, got 2."),
        ([*CH3[:2], "--color", "c.ppm"], "--color needs exactly 3 --channel images, got 1."),
        (["--color"], "Argument --color needs a value."),
        (["--compose", "cmyk"], "Invalid compose mode (want rgb or hsl): cmyk"),
        (["--compose"], "Argument --compose needs a value."),
        (["--hue-shift", "0.3x"], "Invalid number given to argument --hue-shift: 0.3x"),
        (["--hue-shift", "nan"], "Invalid hue shift (want a finite number): nan"),
        (["--color-stretch", "2"], "Invalid color stretch (want B:W, percentages with B + W < 100): 2"),
        (["--color-stretch", "2:"], "Invalid color stretch (want B:W, percentages with B + W < 100): 2:"),
        (["--color-stretch", "a:b"], "Invalid color stretch (want B:W, percentages with B + W < 100): a:b"),
        (["--color-stretch", "60:40"], "Invalid color stretch (want B:W, percentages with B + W < 100): 60:40"),
        (["--color-stretch", "-1:1"], "Invalid color stretch (want B:W, percentages with B + W < 100): -1:1"),
        (["--color-stretch", "inf:0"], "Invalid color stretch (want B:W, percentages with B + W < 100): inf:0"),
        (["--color-stretch", "2:1:0"], "Invalid color stretch (want B:W, percentages with B + W < 100): 2:1:0"),
    ],
)
def test_bad_color_flags_print_message_then_usage_and_exit_zero(exe, args, first_line):
    r = run(exe, *args)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    assert lines[0] == first_line
    assert lines[1] == "Usage: %s [options]" % exe


def test_color_flags_in_any_order_pass_parsing(exe, tmp_path):
    # --color before its channels, every colour flag given: parsing succeeds and the run gets as far as the device
    # (exit 1 without a GPU, 0 with one) -- either way no usage text
    r = run(exe, "--color", str(tmp_path / "c.ppm"), "--compose", "hsl", "--hue-shift", "-1.7", "--color-stretch",
            "0:0", *CH3, "-w", "8", "-h", "8", "--passes", "0", cwd=str(tmp_path))
    assert "Usage:" not in r.stdout
    assert r.stdout.startswith("Creating 8x8 image, 1500 max iterations.\nCalculating image...\n")
