"""The white clip on the device (exposure.hip; include/cudabrot_amd.h, "White clip"): the radix select over
u64 counters equals the host's definition bit for bit -- on the arrays of the host suite and on four more that exist only
to break the kernel --, the clipped tone map equals the host function in all three table forms, and the renderer and the
binary apply it to the array whose maximum they take otherwise."""

import re

import numpy as np
import pytest

import exposure_reference as expo
import plot_reference as plot
from conftest import read_state_file
from output_planted import on_device, source
from plot_harness import DEPTH_SHAPE, exe  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

CASES = expo.cases()
# exposure.hip's launch (counter_sweep.h): kSweepBlocks blocks of kSweepThreads lanes, each lane kLoads loads of kVector
# counters per turn -- one full sweep of the grid is their product
BLOCKS, THREADS, LOADS, VECTOR = 1024, 256, 4, 2
SWEEP = BLOCKS * THREADS * LOADS * VECTOR
MODES = ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"]


def test_the_grid_named_here_is_the_code_s():
    assert source("counter_sweep.h")[1] == {"kSweepBlocks": BLOCKS, "kSweepThreads": THREADS, "kLoads": LOADS, "kVector": VECTOR}
    assert "for_each_counter(hist, n," in source("exposure.hip")[0] and source("exposure.hip")[1] == {}


def device_white_count(cb, values, clip, offset=0):
    import torch

    base, view = on_device(values, offset)
    assert view.data_ptr() % 16 == (8 if offset % 2 else 0)
    got = cb.white_count_device(view.data_ptr(), view.numel(), clip, stream=torch.cuda.current_stream().cuda_stream)
    del base
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_white_count_equals_the_host_s(cb, name):
    hist = CASES[name]
    for clip in expo.CLIPS + (expo.BOUNDARY_CLIPS if name == "rank_on_a_boundary" else ()):
        want = cb.white_count(hist, clip)
        assert want == expo.white_count(hist, clip)
        assert device_white_count(cb, hist, clip) == want, clip


def kernel_breakers():
    rng = np.random.default_rng(5)
    heavy = lambda n: np.minimum((rng.pareto(1.2, size=n) * 3).astype(np.uint64), np.uint64(60_000))  # noqa: E731
    long = heavy(SWEEP + 3)
    long[-1] = 1 << 40      # the last three counters, past the sweep, decide the answers below
    long[-2] = 65_536
    long[-3] = 0
    return {
        "n_1": (np.array([9], dtype=np.uint64), 0),
        "n_2k_plus_1": (np.array([3, 0, 8, 8, 1 << 33], dtype=np.uint64), 0),          # 2 * kVector + 1
        "sweep_plus_3": (long, 0),
        "misaligned": (heavy(4 * THREADS * VECTOR + 2), 1),                             # 8-byte, not 16-byte aligned
        "misaligned_n_1": (np.array([9], dtype=np.uint64), 1),
        "misaligned_even_n": (np.array([5, 6, 7, 1 << 50], dtype=np.uint64), 1),        # a head AND a tail counter
    }


@pytest.mark.parametrize("name", ["n_1", "n_2k_plus_1", "sweep_plus_3", "misaligned", "misaligned_n_1", "misaligned_even_n"])
def test_arrays_made_to_break_the_kernel(cb, name):
    values, offset = kernel_breakers()[name]
    for clip in (0.0, 1e-4, 1.0, 50.0, 99.999999):
        want = cb.white_count(values, clip)
        assert device_white_count(cb, values, clip, offset) == want, clip
    if name == "sweep_plus_3":  # the counters behind the full sweep were read: the maximum and the second largest are there
        assert cb.white_count(values, 0.0)[0] == 1 << 40
        lit = int(np.count_nonzero(values))
        assert device_white_count(cb, values, 100.0 * 1.5 / lit, offset) == (int(np.sort(values)[-2]), lit, 1)


def test_device_white_count_refuses_bad_arguments(cb):
    import ctypes as C

    base, view = on_device(np.arange(8, dtype=np.uint64))
    out = [C.c_uint64(7) for _ in range(3)]
    refs = [C.byref(v) for v in out]
    f = cb.lib.cb_white_count_device
    assert f(None, 8, 1.0, *refs, None) == 1
    assert f(view.data_ptr(), 0, 1.0, *refs, None) == 1
    assert f(view.data_ptr(), (1 << 40) + 1, 1.0, *refs, None) == 1                     # the bound of the u32 bins
    assert f(view.data_ptr() + 4, 4, 1.0, *refs, None) == 1                             # not a u64 address
    for bad in (-1.0, 100.0, float("nan"), float("inf")):
        assert f(view.data_ptr(), 8, bad, *refs, None) == 1
    assert f(view.data_ptr(), 8, 1.0, None, refs[1], refs[2], None) == 1
    assert [v.value for v in out] == [7, 7, 7]
    assert f(view.data_ptr(), 8, 50.0, *refs, None) == 0 and [v.value for v in out] == [4, 7, 3]


def device_tone_map_white(cb, hist, gamma, clip, mode):
    import torch

    h, w = hist.shape
    keep, d_hist = on_device(hist)
    d_gray = torch.zeros(h * w, dtype=torch.int16, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if clip is None:
        mx, scale = cb.tone_map_device(d_hist.data_ptr(), w, h, gamma, d_gray.data_ptr(), mode=mode, stream=stream)
        white = mx
    else:
        mx, scale, white = cb.tone_map_device_white(d_hist.data_ptr(), w, h, gamma, clip, d_gray.data_ptr(), mode=mode,
                                                    stream=stream)
    torch.cuda.synchronize()
    return d_gray.cpu().numpy().view(">u2").reshape(h, w), mx, scale, white


@pytest.mark.parametrize("gamma", expo.GAMMAS)
@pytest.mark.parametrize("mode", MODES)
def test_clipped_device_tone_map_equals_the_host_function(cb, gamma, mode):
    hist = CASES["heavy_tail"]
    body, mx, scale, white = device_tone_map_white(cb, hist, gamma, 0.5, getattr(cb, mode))
    gray, want_max, want_scale, want_white = cb.set_grayscale_pixels_white(hist, gamma, 0.5)
    assert (mx, scale, white) == (want_max, want_scale, want_white) and white < mx == 1_000_003
    assert np.array_equal(body.astype(np.uint16), gray)
    # p = 0: cb_tone_map_device, byte for byte
    zero, mx0, scale0, white0 = device_tone_map_white(cb, hist, gamma, 0.0, getattr(cb, mode))
    plain, want_max0, want_scale0, _ = device_tone_map_white(cb, hist, gamma, None, getattr(cb, mode))
    assert (mx0, scale0, white0) == (want_max0, want_scale0, want_max0)
    assert zero.tobytes() == plain.tobytes()


def test_a_hot_pixel_beyond_the_table_limit_takes_the_table_once_clipped(cb):
    hist = expo.synthetic_histogram(11, 64, 96, 1_000_000)
    hist[5, 5] = (1 << 37) + 12345
    with pytest.raises(cb.CudabrotError):  # unclipped, a 2^37-entry table is refused (tests/test_gpu_tonemap.py)
        device_tone_map_white(cb, hist, 1.0, None, cb.CB_TONE_LUT)
    for gamma in (1.0, 2.2):
        for mode in MODES:
            body, mx, scale, white = device_tone_map_white(cb, hist, gamma, 1.0, getattr(cb, mode))
            gray, want_max, want_scale, want_white = cb.set_grayscale_pixels_white(hist, gamma, 1.0)
            assert mx == want_max == (1 << 37) + 12345 and white == want_white < (1 << 24) and scale == want_scale
            assert np.array_equal(body.astype(np.uint16), gray)
            assert int(body[5, 5]) == cb.tone_value(white, white, gamma)
    # all zeros: white 0, scale inf, a zero image, as unclipped
    body, mx, scale, white = device_tone_map_white(cb, CASES["all_zero"], 1.0, 1.0, cb.CB_TONE_AUTO)
    assert (mx, white) == (0, 0) and scale == float("inf") and not body.any()


def test_renderer_grayscale_image_with_a_clip(cb):
    dims = cb.FractalDimensions.make(320, 240)
    with cb.Renderer(dims, cb.IterationControl(300, 20), n_threads=8192) as r:
        r.render_passes(3)
        assert r.white_clip == 0.0 and r.last_white() == (0, 0, 0)
        plain, plain_max, plain_scale = r.grayscale_image(2.2)
        assert r.last_white() == (0, 0, 0)
        r.set_white_clip(1.0)
        assert r.white_clip == 1.0
        body, mx, scale = r.grayscale_image(2.2)
        hist = r.read_histogram()
        gray, want_max, want_scale, want_white = cb.set_grayscale_pixels_white(hist, 2.2, 1.0)
        assert (mx, scale) == (want_max, want_scale) and mx == plain_max and want_white < mx
        assert np.array_equal(body.astype(np.uint16), gray)
        assert r.last_white() == cb.white_count(hist, 1.0) == expo.white_count(hist, 1.0)
        assert r.last_white()[0] == want_white
        # a bad value is refused and leaves the renderer as it was
        for bad in (-1.0, 100.0, float("nan")):
            assert cb.lib.cb_renderer_set_white_clip(r._h, bad) == 1
        assert r.white_clip == 1.0 and r.last_white()[0] == want_white
        # a clipped renderer makes no colour image
        with pytest.raises(cb.CudabrotError):
            r.color_image((0, 0, 0))
        # the clip is an output setting: the histogram is what it was, and 0 gives the unclipped bytes again
        assert np.array_equal(r.read_histogram(), hist)
        r.set_white_clip(0)
        again, again_max, again_scale = r.grayscale_image(2.2)
        assert (again_max, again_scale) == (plain_max, plain_scale) and again.tobytes() == plain.tobytes()
        assert r.last_white() == (0, 0, 0)
        rgb, _ = r.color_image((0, 0, 0))
        assert rgb.shape == (240, 320, 3)


def check_common_white(cb, hist, clip, found):
    """`found` is the white point over ALL planes as one array, and no plane's own for at least one plane."""
    assert found == expo.white_count(hist, clip) == cb.white_count(hist, clip)
    own = [expo.white_count(p, clip)[0] for p in hist]
    assert any(w != found[0] for w in own), (own, found)


def test_palette_renderer_shares_one_white_among_its_planes(cb):
    w, h = 64, 48
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(500, 20), device=0, n_threads=1000) as r:
        r.set_palette(plot.demo_table(500))
        r.render_passes(3)
        plain, plain_max, _ = r.palette_image(2.2)
        r.set_white_clip(1.0)
        rgb, mx, scale = r.palette_image(2.2)
        hist = r.read_histogram()
        assert hist.shape == (3, h, w)
        check_common_white(cb, hist, 1.0, r.last_white())
        planar, want_max, want_scale, white = cb.set_grayscale_pixels_white(hist.reshape(3 * h, w), 2.2, 1.0)
        assert (mx, scale) == (want_max, want_scale) and mx == plain_max and white == r.last_white()[0]
        want = np.ascontiguousarray(planar.reshape(3, h, w).transpose(1, 2, 0)).astype(">u2")
        assert rgb.shape == (h, w, 3) and rgb.tobytes() == want.tobytes()
        # each plane alone has a white of its own
        for j in range(3):
            gray, _, _ = r.grayscale_image(2.2, plane=j)
            assert np.array_equal(gray.astype(np.uint16), cb.set_grayscale_pixels_white(hist[j], 2.2, 1.0)[0])
            assert r.last_white() == cb.white_count(hist[j], 1.0)
        r.set_white_clip(0)
        assert r.palette_image(2.2)[0].tobytes() == plain.tobytes()


def test_depth_renderer_shares_one_white_among_its_planes(cb):
    w, h, max_iter, min_iter, threads, _ = DEPTH_SHAPE
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(max_iter, min_iter), device=0, n_threads=threads) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 3))
        r.render_passes(3)
        plain, plain_max, _ = r.depth_image(1.0)
        r.set_white_clip(1.0)
        gray, mx, scale = r.depth_image(1.0)
        hist = r.read_histogram()
        assert hist.shape == (3, h, w)
        check_common_white(cb, hist, 1.0, r.last_white())
        want, want_max, want_scale, white = cb.set_grayscale_pixels_white(hist.reshape(3 * h, w), 1.0, 1.0)
        assert (mx, scale) == (want_max, want_scale) and mx == plain_max and white == r.last_white()[0]
        assert gray.shape == (3, h, w) and np.array_equal(gray.astype(np.uint16).reshape(3 * h, w), want)
        r.set_white_clip(0)
        assert r.depth_image(1.0)[0].tobytes() == plain.tobytes()


def test_cli_white_clip_host_and_device_files_and_the_line(cb, exe, tmp_path):  # noqa: F811
    common = ["--bounded", "--julia", "-1,0", "-m", "500", "-w", "64", "-h", "48", "--passes", "2"]
    files = {k: (str(tmp_path / (k + ".pgm")), str(tmp_path / (k + ".bin"))) for k in ("device", "host", "plain")}
    runs = {
        "device": run(exe, *common, "--white-clip", "1", "-o", files["device"][0], "-s", files["device"][1]),
        "host": run(exe, *common, "--white-clip", "1", "--tonemap", "host", "-o", files["host"][0], "-s", files["host"][1]),
        "plain": run(exe, *common, "-o", files["plain"][0], "-s", files["plain"][1]),
    }
    for k, r in runs.items():
        assert r.returncode == 0, r.stdout + r.stderr
    hist = read_state_file(files["device"][1], 48, 64)
    assert np.array_equal(read_state_file(files["host"][1], 48, 64), hist)
    assert np.array_equal(read_state_file(files["plain"][1], 48, 64), hist)  # the clip touches no histogram
    white, lit, clipped = cb.white_count(hist, 1.0)
    assert 0 < white < int(hist.max()) and clipped > 0
    for k in ("device", "host"):
        lines = runs[k].stdout.split("\n")
        at = [i for i, line in enumerate(lines) if line.startswith("White value:")]
        assert len(at) == 1 and lines[at[0] - 1].startswith("Max value: %d, scale: " % int(hist.max())), runs[k].stdout
        assert lines[at[0] - 1] == "Max value: %d, scale: %f" % (int(hist.max()), 65535.0 / white)
        m = re.fullmatch(r"White value: (\d+) \((\S+)% of (\d+) lit pixels may clip, (\d+) do\)", lines[at[0]])
        assert m and (int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))) == (white, "1", lit, clipped), lines[at[0]]
    assert "White value" not in runs["plain"].stdout
    body = {k: open(files[k][0], "rb").read() for k in files}
    assert body["device"] == body["host"] != body["plain"]
    gray = cb.set_grayscale_pixels_white(hist, 1.0, 1.0)[0]
    assert body["device"] == b"P5\n64 48\n65535\n" + gray.astype(">u2").tobytes()
