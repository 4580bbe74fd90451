"""The equalised image on the device (equalize.hip; include/cudabrot_amd.h, "Equalised image"): the one
sweep into 56 320 bins equals the host's definition bit for bit -- on the arrays of the host suite and on more that exist
only to break the kernel --, the mapped image equals the host function's bytes, and the renderer and the binary apply it
to the array whose maximum they take otherwise."""

import ctypes as C

import numpy as np
import pytest

import equalize_reference as eq
import plot_reference as plot
from conftest import read_state_file
from output_planted import on_device, source
from plot_harness import DEPTH_SHAPE, exe  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

CASES = eq.cases()
INVALID = 1  # hipErrorInvalidValue
# equalize.hip's launch (counter_sweep.h): kSweepBlocks blocks of kSweepThreads lanes, each lane kLoads loads of kVector
# counters per turn -- one full sweep of the grid is their product; keys below equalize.hip's kWindow are counted in LDS,
# the others in global memory
BLOCKS, THREADS, LOADS, VECTOR, WINDOW = 1024, 256, 4, 2, 8192
SWEEP = BLOCKS * THREADS * LOADS * VECTOR
BLOCK_TURN = THREADS * LOADS * VECTOR
MODES = ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"]
FILTER = (4, 0.5, 2)


def test_the_grid_named_here_is_the_code_s():
    assert source("counter_sweep.h")[1] == {"kSweepBlocks": BLOCKS, "kSweepThreads": THREADS, "kLoads": LOADS, "kVector": VECTOR}
    assert "for_each_counter(hist, n," in source("equalize.hip")[0] and source("equalize.hip")[1] == {"kWindow": WINDOW}


def device_bins(cb, values, offset=0):
    import torch

    base, view = on_device(values, offset)
    assert view.data_ptr() % 16 == (8 if offset % 2 else 0)
    got = cb.equalize_bins_device(view.data_ptr(), view.numel(), stream=torch.cuda.current_stream().cuda_stream)
    del base
    return got


def same_bins(got, want):
    assert got[1:] == want[1:], (got[1:], want[1:])
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_bins_lit_and_max_equal_the_host_s(cb, name):
    want = cb.equalize_bins(CASES[name])
    same_bins(want, eq.bins(CASES[name]))
    same_bins(device_bins(cb, CASES[name]), want)


def breakers():
    """name -> (counters, offset of the base pointer in counters)."""
    rng = np.random.default_rng(5)
    long = eq.heavy(rng, SWEEP + 3)
    long[long == 2047] += np.uint64(1)
    long[-1] = 1 << 40      # the last three counters, past the sweep, decide the answers below
    long[-2] = 2047         # (the only one)
    long[-3] = 0
    below, at = eq.lowest_count(WINDOW - 1), eq.lowest_count(WINDOW)
    side_by_side = np.where(np.arange(BLOCK_TURN + 6) % 2 == 0, at - 1, at).astype(np.uint64)
    return {
        "n_1": (np.array([9], dtype=np.uint64), 0),
        "n_2k_plus_1": (np.array([3, 0, 8, 8, 1 << 33], dtype=np.uint64), 0),          # 2 * kVector + 1
        "sweep_plus_3": (long, 0),
        "misaligned_n_1": (np.array([9], dtype=np.uint64), 1),                          # 8-byte, not 16-byte aligned
        "misaligned_even_n": (np.array([5, 6, 7, 1 << 50], dtype=np.uint64), 1),        # a head AND a tail counter
        "misaligned_odd_n": (eq.heavy(rng, 4 * THREADS * VECTOR + 3, 1 << 20), 1),
        "crowded_below_window": (np.full(BLOCK_TURN, below, dtype=np.uint64), 0),       # one LDS bin takes a block's worth
        "crowded_at_window": (np.full(BLOCK_TURN, at, dtype=np.uint64), 0),             # one global bin does
        "crowded_far_above_window": (np.full(BLOCK_TURN, (1 << 64) - 1, dtype=np.uint64), 0),
        "window_edge_side_by_side": (side_by_side, 0),                                  # keys W - 1 and W, lane by lane
    }


BREAKERS = breakers()


@pytest.mark.parametrize("name", sorted(BREAKERS))
def test_arrays_made_to_break_the_kernel(cb, name):
    values, offset = BREAKERS[name]
    want = cb.equalize_bins(values)
    got = device_bins(cb, values, offset)
    same_bins(got, want)
    if name == "sweep_plus_3":  # the counters behind the full sweep were read: the maximum and the only 2047 are there
        assert got[2] == 1 << 40 and int(got[0][2047]) == 1 and int(got[0][eq.key(1 << 40)]) == 1
        assert got[1] == int(np.count_nonzero(values))
    if name.startswith("crowded"):
        assert np.count_nonzero(got[0]) == 1 and int(got[0].max()) == BLOCK_TURN
    if name == "window_edge_side_by_side":
        assert (eq.key(int(values[0])), eq.key(int(values[1]))) == (WINDOW - 1, WINDOW)
        assert [int(got[0][WINDOW - 1]), int(got[0][WINDOW])] == [BLOCK_TURN // 2 + 3] * 2


def test_device_bins_refuse_bad_arguments_with_nothing_written(cb):
    base, view = on_device(np.arange(8, dtype=np.uint64))
    bins = np.full(eq.KEYS, 77, dtype=np.uint64)
    out = [C.c_uint64(7) for _ in range(2)]
    refs = [C.byref(v) for v in out]
    f = cb.lib.cb_equalize_bins_device
    p, b = view.data_ptr(), bins.ctypes.data
    assert f(None, 8, b, *refs, None) == INVALID
    assert f(p, 0, b, *refs, None) == INVALID
    assert f(p, (1 << 40) + 1, b, *refs, None) == INVALID                               # the bound of the u32 bins
    assert f(p + 4, 4, b, *refs, None) == INVALID                                       # not a u64 address
    assert f(p, 8, None, *refs, None) == INVALID
    assert f(p, 8, b, None, refs[1], None) == INVALID
    assert f(p, 8, b, refs[0], None, None) == INVALID
    assert [v.value for v in out] == [7, 7] and set(bins.tolist()) == {77}
    assert f(p, 8, b, *refs, None) == 0 and [v.value for v in out] == [7, 7] and bins[1:8].tolist() == [1] * 7


def device_image(cb, hist, gamma):
    import torch

    h, w = hist.shape
    keep, d_hist = on_device(hist)
    d_gray = torch.zeros(h * w + 2, dtype=torch.int16, device="cuda:0")  # (two spare values behind)
    numbers = cb.tone_map_device_equalized(d_hist.data_ptr(), w, h, gamma, d_gray.data_ptr(),
                                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_gray.cpu().numpy()
    assert not got[h * w:].any()
    return got[:h * w].view(">u2").reshape(h, w), numbers


@pytest.mark.parametrize("gamma", [2.2, 1.0, 0.0])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (1, 63), DEPTH_SHAPE[1::-1]])
def test_device_image_bytes_equal_the_host_function_s(cb, shape, gamma):
    h, w = shape
    hist = eq.heavy(np.random.default_rng(h * w), h * w, 1 << 36).reshape(h, w) + np.uint64(h * w == 1)
    body, (mx, scale, lit, keys, levels) = device_image(cb, hist, gamma)
    gray, want_max, want_scale, want_lit = cb.set_grayscale_pixels_equalized(hist, gamma)
    assert (mx, scale, lit) == (want_max, want_scale, want_lit) and lit > 0
    assert (keys, levels) == cb.equalize_table(cb.equalize_bins(hist)[0], gamma)[1:]
    assert body.tobytes() == gray.astype(">u2").tobytes()


def test_device_image_of_the_shared_cases_and_its_refusals(cb):
    import torch

    for name in ("all_zero", "key_edges", "u64_max", "colour_planes"):
        body, numbers = device_image(cb, CASES[name], 2.2)
        gray, mx, scale, lit = cb.set_grayscale_pixels_equalized(CASES[name], 2.2)
        assert body.tobytes() == gray.astype(">u2").tobytes(), name
        assert numbers[0] == mx and numbers[2] == lit and (numbers[1] == scale or mx == 0), name
    keep, d_hist = on_device(np.arange(8, dtype=np.uint64))
    d_gray = torch.full((8,), 0x77, dtype=torch.int16, device="cuda:0")
    f = cb.lib.cb_tone_map_device_equalized
    p, g = d_hist.data_ptr(), d_gray.data_ptr()
    for call in [(None, 4, 2, 1.0, g), (p, 4, 2, 1.0, None), (p, 0, 2, 1.0, g), (p, 4, -2, 1.0, g), (p + 4, 2, 2, 1.0, g),
                 (p, 1 << 21, 1 << 20, 1.0, g)]:
        assert f(*call, None, None, None, None, None, None) == INVALID, call
    torch.cuda.synchronize()
    assert (d_gray.cpu().numpy() == 0x77).all()
    assert f(p, 4, 2, 1.0, g, None, None, None, None, None, None) == 0  # every output number is optional


# ---- the renderer: every image call takes the equalised map over the array it takes the maximum of ----


def host_rows(cb, hist, group, gamma, filtered):
    """The host definition over a histogram [h, w] or [planes, h, w] as one image -> (u16 [rows, w], max, scale, numbers)."""
    if filtered:
        hist = cb.density_filter(hist, cb.density_thresholds(*FILTER), group)
    rows = hist.reshape(-1, hist.shape[-1])
    gray, mx, scale, lit = cb.set_grayscale_pixels_equalized(rows, gamma)
    want, want_lit, keys, levels = eq.image(cb, rows, gamma)
    assert gray.tobytes() == want.tobytes() and lit == want_lit > 0
    assert (mx, scale) == cb.set_grayscale_pixels(rows, gamma)[1:]  # what the unflagged call returns
    return gray, mx, scale, (lit, keys, levels)


def check_images(cb, r, image, group, shape_out, pick=lambda planes: planes):
    """`image(gamma, mode)` of a rendered renderer `r`, equalised: plain and over the filtered counters, in every mode;
    `pick` takes the planes the image is made of out of the histogram read back."""
    hist = pick(r.read_histogram())
    plain, plain_max, plain_scale = image(2.2, 0)
    assert not r.equalize and r.last_equalize() == (0, 0, 0)
    r.set_equalize()
    assert r.equalize and r.last_equalize() == (0, 0, 0)
    for filtered in (False, True):
        r.set_density_filter(*(FILTER if filtered else (0,)))
        for gamma in (2.2, 0.0):
            want, want_max, want_scale, numbers = host_rows(cb, hist, group, gamma, filtered)
            for mode in MODES:
                got, mx, scale = image(gamma, getattr(cb, mode))
                assert (mx, scale) == (want_max, want_scale), (filtered, gamma, mode)
                assert np.array_equal(shape_out(got.astype(np.uint16)), want), (filtered, gamma, mode)
                assert r.last_equalize() == numbers
        if not filtered:
            assert (want_max, want_scale) == (plain_max, plain_scale)
    r.set_density_filter(0)
    # the mode is validated; a clip on an equalised renderer is refused and changes nothing; a clip of 0 is no clip
    with pytest.raises(cb.CudabrotError):
        image(2.2, 7)
    before = r.last_equalize()
    assert cb.lib.cb_renderer_set_white_clip(r._h, 1.0) == INVALID and r.white_clip == 0.0 and r.equalize
    assert cb.lib.cb_renderer_set_white_clip(r._h, 0.0) == 0 and r.last_equalize() == before
    # an output setting: the histogram is what it was, and clearing it gives the unflagged bytes again
    assert np.array_equal(pick(r.read_histogram()), hist)
    r.set_equalize(False)
    assert not r.equalize and r.last_equalize() == (0, 0, 0)
    again, again_max, again_scale = image(2.2, 0)
    assert (again_max, again_scale) == (plain_max, plain_scale) and again.tobytes() == plain.tobytes()
    assert r.last_equalize() == (0, 0, 0)
    # ... and equalisation on a clipped renderer is refused, the clip staying
    r.set_white_clip(1.0)
    clipped = image(2.2, 0)[0].tobytes()
    found = r.last_white()
    assert cb.lib.cb_renderer_set_equalize(r._h, 1) == INVALID
    assert not r.equalize and r.white_clip == 1.0 and r.last_white() == found and image(2.2, 0)[0].tobytes() == clipped
    assert cb.lib.cb_renderer_set_equalize(r._h, 0) == 0 and r.white_clip == 1.0
    r.set_white_clip(0)


def test_grey_renderer(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 48), cb.IterationControl(300, 20), n_threads=2048) as r:
        r.render_passes(3)
        check_images(cb, r, lambda g, m: r.grayscale_image(g, m), 1, lambda a: a)
        r.set_equalize()
        with pytest.raises(cb.CudabrotError):  # an equalised renderer makes no colour image
            r.color_image((0, 0, 0))
        r.set_equalize(False)
        assert r.color_image((0, 0, 0))[0].shape == (48, 64, 3)


def test_channel_renderer_equalises_each_plane_on_its_own(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 48), [(300, 20), (60, 10)], n_threads=2048) as r:
        r.render_passes(3)
        hist = r.read_histogram()
        assert hist.shape == (2, 48, 64)
        for plane in (0, 1):  # everything the other renders are held to, on one plane at its offset in the histogram
            check_images(cb, r, lambda g, m, plane=plane: r.grayscale_image(g, m, plane=plane), 1, lambda a: a,
                         pick=lambda planes, plane=plane: planes[plane])
        assert host_rows(cb, hist[0], 1, 2.2, False)[3] != host_rows(cb, hist[1], 1, 2.2, False)[3]


def test_palette_renderer_shares_one_table_among_its_planes(cb):
    w, h = 64, 48
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(500, 20), device=0, n_threads=1000) as r:
        r.set_palette(plot.demo_table(500))
        r.render_passes(3)
        assert r.read_histogram().shape == (3, h, w)
        check_images(cb, r, r.palette_image, 3, lambda a: a.transpose(2, 0, 1).reshape(3 * h, w))


def test_depth_renderer_shares_one_table_among_its_slices(cb):
    w, h, max_iter, min_iter, threads, _ = DEPTH_SHAPE
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(max_iter, min_iter), device=0, n_threads=threads) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 3))
        r.render_passes(3)
        hist = r.read_histogram()
        assert hist.shape == (3, h, w)
        check_images(cb, r, r.depth_image, 1, lambda a: a.reshape(3 * h, w))
        # one table over all slices is no slice's own
        shared = cb.set_grayscale_pixels_equalized(hist.reshape(3 * h, w), 2.2)[0].reshape(3, h, w)
        assert any(not np.array_equal(shared[s], cb.set_grayscale_pixels_equalized(hist[s], 2.2)[0]) for s in range(3))


def test_frames_renderer_shares_one_table_among_its_frames(cb):
    w, h, max_iter, min_iter, threads, _ = DEPTH_SHAPE
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(max_iter, min_iter), device=0, n_threads=threads) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_frames(cb.frames_from_sweep(cb.IDENTITY_PROJECTION, ("zr", "cr"), 0.0, 90.0, 2)[0])
        r.render_passes(3)
        assert r.read_histogram().shape == (2, h, w)
        check_images(cb, r, r.frames_image, 1, lambda a: a.reshape(2 * h, w))


# ---- the binary ----


CLI_COMMON = ["-m", "300", "-w", "64", "-h", "48", "--passes", "2", "-g", "0.5", "--stats", "--kernel", "simple"]
HEADER = b"P5\n64 48\n65535\n"


def cli_runs(exe, tmp_path, forms):  # noqa: F811
    """name -> (the finished run, its image file, its -s file) of CLI_COMMON + forms[name]."""
    out = {}
    for k, more in forms.items():
        image, state = str(tmp_path / (k + ".pgm")), str(tmp_path / (k + ".bin"))
        r = run(exe, *CLI_COMMON, *more, "-o", image, "-s", state)
        assert r.returncode == 0, r.stdout + r.stderr
        out[k] = (r, image, state)
    return out


def test_cli_writes_one_file_in_every_tone_form_and_says_what_it_found(cb, exe, tmp_path):  # noqa: F811
    runs = cli_runs(exe, tmp_path, {k: ["--equalize", "--tonemap", k] for k in ("lut", "thresholds", "host")})
    hist = read_state_file(runs["lut"][2], 48, 64)
    gray, mx, scale, lit = cb.set_grayscale_pixels_equalized(hist, 0.5)
    _, keys, levels = cb.equalize_table(cb.equalize_bins(hist)[0], 0.5)
    line = "Equalized: %d lit pixels in %d keys, %d output levels" % (lit, keys, levels)
    assert lit > 0 and keys > 1 and levels > 1
    for k, (r, image, state) in runs.items():
        assert open(image, "rb").read() == HEADER + gray.astype(">u2").tobytes(), k
        assert np.array_equal(read_state_file(state, 48, 64), hist), k
        lines = r.stdout.split("\n")
        at = [i for i, said in enumerate(lines) if said.startswith("Equalized:")]
        assert len(at) == 1 and lines[at[0]] == line, r.stdout
        assert lines[at[0] - 1] == "Max value: %d, scale: %f" % (mx, scale), k              # what it is without the flag
        assert [said for said in r.stderr.split("\n") if "equalize" in said] == ['{"equalize": true}'], k


def test_cli_without_the_flag_is_what_it_was(cb, exe, tmp_path):  # noqa: F811
    """The file and stdout of the parent behaviour, which --tonemap host restates; the flag touches no -s file and adds its
    one line to stdout and nothing else (the line that carries a time apart)."""
    runs = cli_runs(exe, tmp_path, {"plain": [], "plain_host": ["--tonemap", "host"], "host": ["--equalize", "--tonemap", "host"]})
    hist = read_state_file(runs["plain"][2], 48, 64)
    gray, mx, scale = cb.set_grayscale_pixels(hist, 0.5)
    plain = open(runs["plain"][1], "rb").read()
    assert plain == open(runs["plain_host"][1], "rb").read() == HEADER + gray.astype(">u2").tobytes()
    assert open(runs["host"][1], "rb").read() != plain
    assert open(runs["host"][2], "rb").read() == open(runs["plain"][2], "rb").read() == open(runs["plain_host"][2], "rb").read()
    for k in ("plain", "plain_host"):
        assert "Equalized" not in runs[k][0].stdout and "equalize" not in runs[k][0].stderr
        assert "Max value: %d, scale: %f" % (mx, scale) in runs[k][0].stdout.split("\n")

    def said(k):
        r, image, state = runs[k]
        lines = [s.replace(image, "FILE").replace(state, "STATE") for s in r.stdout.split("\n")]
        return [s for s in lines if " passes took " not in s and not s.startswith("Equalized:")]

    assert said("plain_host") == said("host") and len(said("host")) == len(runs["host"][0].stdout.split("\n")) - 2


def test_cli_equalizes_the_filtered_counters_of_a_stack(cb, exe, tmp_path):  # noqa: F811
    common = ["-m", "300", "-w", "64", "-h", "48", "--passes", "2", "--depth", "cr:-2:0.5:3", "--density-filter", "4:0.5:2",
              "--equalize", "-g", "2.2"]
    bodies, outs = {}, {}
    for k, more in {"device": [], "host": ["--tonemap", "host"]}.items():
        r = run(exe, *common, *more, "-o", str(tmp_path / (k + ".pgm")), "-s", str(tmp_path / (k + ".bin")))
        assert r.returncode == 0, r.stdout + r.stderr
        bodies[k] = open(tmp_path / (k + ".pgm"), "rb").read()
        outs[k] = [line for line in r.stdout.split("\n") if line.startswith(("Max value", "Density filter", "Equalized"))]
    hist = read_state_file(str(tmp_path / "device.bin"), 48, 64, planes=3)
    filtered = cb.density_filter(hist, cb.density_thresholds(4, 0.5, 2)).reshape(3 * 48, 64)
    gray, mx, scale, lit = cb.set_grayscale_pixels_equalized(filtered, 2.2)
    _, keys, levels = cb.equalize_table(cb.equalize_bins(filtered)[0], 2.2)
    header = b"P5\n64 48\n65535\n"
    want = b"".join(header + gray[s * 48:(s + 1) * 48].astype(">u2").tobytes() for s in range(3))
    assert bodies["device"] == bodies["host"] == want
    assert outs["device"] == outs["host"] == [
        "Max value: %d, scale: %f" % (mx, scale),
        "Density filter: radius 4, alpha 0.5, n0 2 (the values above carry 8 fraction bits)",
        "Equalized: %d lit pixels in %d keys, %d output levels" % (lit, keys, levels)]
