"""The density filter on the device (density.hip; include/cudabrot_amd.h, "Density filter"): the gather
kernel equals the host's definition and the restatement in Python integers bit for bit -- on the arrays of the host suite
and on shapes that exist only to break the kernel --, the renderer's image calls map the filtered counters, in groups as
the definition says, and the binary writes one file whatever form of tone map it is told to use."""

import ctypes as C
import json

import numpy as np
import pytest

import density_reference as dens
import output_planted
import plot_reference as plot
from conftest import read_state_file
from plot_harness import exe  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

CASES = dens.cases()
TILE_W, TILE_H, THREADS = 64, 16, 256  # density.hip's tile: one workgroup per TILE_W x TILE_H output pixels of a plane
MODES = ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"]
INVALID = 1  # hipErrorInvalidValue


def test_the_tile_named_here_is_the_code_s():
    said = output_planted.source("density.hip")[1]
    assert {k: said[k] for k in ("kTileW", "kTileH", "kDensityThreads")} == {"kTileW": TILE_W, "kTileH": TILE_H, "kDensityThreads": THREADS}


def on_device(values, offset=0, fill=0):
    return output_planted.on_device(values, offset, fill, spare=1)  # (one spare counter behind)


def device_filter(cb, hist, table, group=1, offset=0):
    """cb_density_filter_device on a copy of `hist`; the counters around the output are looked at too."""
    import torch

    a = np.ascontiguousarray(hist, dtype=np.uint64)
    planes, h, w = (1,) + a.shape if a.ndim == 2 else a.shape
    keep_in, d_in = on_device(a, offset)
    keep_out, d_out = on_device(np.full(a.size, 0x7777, dtype=np.uint64), offset, fill=0x5555)
    assert d_in.data_ptr() % 16 == d_out.data_ptr() % 16 == (8 if offset % 2 else 0)
    cb.density_filter_device(d_in.data_ptr(), w, h, planes, group, table, d_out.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    around = keep_out.cpu().numpy()
    assert (around[:offset] == 0x5555).all() and around[-1] == 0x5555          # nothing written outside the planes
    assert np.array_equal(keep_in.cpu().numpy()[offset:-1].view(np.uint64), a.reshape(-1))  # the input is as it was
    return d_out.cpu().numpy().view(np.uint64).reshape(a.shape)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_equals_restatement_on_the_host_suite_s_arrays(cb, name):
    hist, group, params = CASES[name]
    table = cb.density_thresholds(*params)
    want = cb.density_filter(hist, table, group)
    assert np.array_equal(want, dens.expected(name))
    assert np.array_equal(device_filter(cb, hist, table, group), want)


def corner_impulses():
    """R = 8 impulses on the four corners of one inner tile and of the plane: every halo of the tile's neighbours holds one."""
    w, h = 2 * TILE_W + 5, 2 * TILE_H + 3
    a = np.zeros((h, w), dtype=np.uint64)
    for y in (0, TILE_H, 2 * TILE_H - 1, h - 1):
        for x in (0, TILE_W, 2 * TILE_W - 1, w - 1):
            if (y in (0, h - 1)) == (x in (0, w - 1)):
                a[y, x] = 1
    assert np.count_nonzero(a) == 8
    return a


def breakers():
    """name -> (counters, group, (R, alpha, n0), offset of the base pointer in counters)."""
    odd = dens.heavy_tail(2, 3 * 21, 33).reshape(3, 21, 33)  # w * h = 693: planes 1 and 2 start 8 bytes off a 16-byte line
    out = {
        "1x1": (np.array([[1]], dtype=np.uint64), 1, (8, 0.5, 1), 0),
        "1x1_sharp": (np.array([[65]], dtype=np.uint64), 1, (8, 0.5, 1), 0),
        "1x40": (dens.heavy_tail(3, 1, 40), 1, (8, 0.5, 1), 0),
        "40x1": (dens.heavy_tail(3, 40, 1), 1, (8, 0.5, 1), 0),
        "tile_plus_one": (dens.heavy_tail(4, TILE_H + 1, TILE_W + 1), 1, (4, 0.5, 1), 0),
        "tile_plus_one_r8": (dens.heavy_tail(4, TILE_H + 1, TILE_W + 1), 1, (8, 0.5, 1), 0),
        "corner_impulses": (corner_impulses(), 1, (8, 0.5, 1), 0),
        "odd_planes_group_3": (odd, 3, (4, 0.5, 4), 0),
        "odd_planes_group_1": (odd, 1, (4, 0.5, 4), 0),
        "base_8_bytes_in": (dens.heavy_tail(6, 19, 35), 1, (4, 0.5, 1), 1),
        "base_8_bytes_in_group_3": (odd, 3, (8, 0.5, 1), 1),
    }
    for radius in (1, 4, 8):
        out["heavy_tail_97x83_r%d" % radius] = (dens.heavy_tail(8, 83, 97), 1, (radius, 0.5, 1), 0)
    return out


BREAKERS = breakers()


@pytest.mark.parametrize("name", sorted(BREAKERS))
def test_shapes_made_to_break_the_kernel(cb, name):
    hist, group, params, offset = BREAKERS[name]
    table = cb.density_thresholds(*params)
    want = cb.density_filter(hist, table, group)
    assert np.array_equal(want, dens.density_filter(hist, dens.thresholds(*params), group))
    got = device_filter(cb, hist, table, group, offset)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if name == "corner_impulses":  # the plane's corner holds a clipped copy of one blob
        blob = dens.density_filter(np.pad(np.ones((1, 1), dtype=np.uint64), 8), dens.thresholds(*params))
        assert np.array_equal(got[:9, :9], blob[8:, 8:]) and got[0, 0] == blob[8, 8] > 0
    if name.startswith("heavy_tail_97x83"):  # every radius the table can give occurs
        assert ({dens.radius_of(int(c), table) for c in hist[hist > 0]}
                == {dens.radius_of(k, table) for k in range(1, table[1] + 2)})


def test_device_filter_refusals_write_nothing(cb):
    import torch

    table = dens.thresholds(4, 0.5, 1)
    t = (C.c_uint64 * 5)(*table)
    hist = dens.huge_beside_one()
    hist[7, 7] = 1 << 55
    keep_in, d_in = on_device(hist)
    keep_out, d_out = on_device(np.full(64, 0x7777, dtype=np.uint64))
    f = cb.lib.cb_density_filter_device
    stream = torch.cuda.current_stream().cuda_stream
    i, o = d_in.data_ptr(), d_out.data_ptr()
    assert f(i, 8, 8, 1, 1, 4, t, o, stream) == INVALID                 # a counter of 2^55
    for call in [(None, 8, 8, 1, 1, 4, t, o), (i, 8, 8, 1, 1, 4, t, None), (i, 8, 8, 1, 1, 4, t, i), (i, 8, 8, 1, 1, 4, t, i + 8),
                 (i, 0, 8, 1, 1, 4, t, o), (i, 8, 8, 1, 3, 4, t, o), (i, 8, 8, 1, 2, 4, t, o), (i, 8, 8, 1, 1, 0, t, o),
                 (i, 8, 8, 1, 1, 9, t, o), (i + 4, 4, 4, 1, 1, 4, t, o), (i, 4, 4, 1, 1, 4, t, o + 4),
                 (i, 8, 8, 1, 1, 4, (C.c_uint64 * 5)(0, 64, 16, 7, 4), o)]:
        assert f(*call, stream) == INVALID, call
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x7777).all()
    hist[7, 7] = (1 << 55) - 1
    d_in.copy_(torch.from_numpy(hist.reshape(-1).view(np.int64)))
    assert f(i, 8, 8, 1, 1, 4, t, o, stream) == 0
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(8, 8), cb.density_filter(hist, table))


# ---- the renderer: every image call maps the filtered counters ----

FILTER = (4, 0.5, 2)


def host_image(cb, hist, group, gamma, clip):
    """Host filter + host tone map of a histogram [h, w] or [planes, h, w] as one image -> (u16 [rows, w], max, scale)."""
    filtered = cb.density_filter(hist, cb.density_thresholds(*FILTER), group)
    rows = filtered.reshape(-1, filtered.shape[-1])
    if clip:
        gray, mx, scale, _ = cb.set_grayscale_pixels_white(rows, gamma, clip)
    else:
        gray, mx, scale = cb.set_grayscale_pixels(rows, gamma)
    assert mx == int(filtered.max()) and mx > 0
    return gray, mx, scale


def check_images(cb, r, image, group, shape_out):
    """`image(gamma, mode)` of a rendered renderer `r` with the filter, over the three modes, with and without a clip."""
    hist = r.read_histogram()
    plain, plain_max, _ = image(2.2, 0)
    assert r.density_filter == (0, 0.0, 0)
    r.set_density_filter(*FILTER)
    assert r.density_filter == FILTER
    for clip in (0.0, 2.0):
        r.set_white_clip(clip)
        for gamma in (2.2, 1.0):
            want, want_max, want_scale = host_image(cb, hist, group, gamma, clip)
            for mode in MODES:
                got, mx, scale = image(gamma, getattr(cb, mode))
                assert (mx, scale) == (want_max, want_scale), (clip, gamma, mode)
                assert np.array_equal(shape_out(got.astype(np.uint16)), want), (clip, gamma, mode)
        if clip:  # the white point is taken from the filtered values
            filtered = cb.density_filter(hist, cb.density_thresholds(*FILTER), group)
            assert r.last_white() == cb.white_count(filtered, clip)
    # an output setting: the histogram is what it was, bad parameters leave it as it is, radius 0 gives the plain bytes again
    assert np.array_equal(r.read_histogram(), hist)
    for bad in ((9, 0.5, 1), (4, 0.01, 1), (4, 0.5, 0), (8, 0.0625, 1), (-1, 0.5, 1)):
        assert cb.lib.cb_renderer_set_density_filter(r._h, *bad) == INVALID
    assert r.density_filter == FILTER
    r.set_white_clip(0)
    r.set_density_filter(0)
    again, again_max, _ = image(2.2, 0)
    assert again_max == plain_max and again.tobytes() == plain.tobytes()


def test_grey_renderer_maps_the_filtered_counters(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 64), cb.IterationControl(300, 20), n_threads=2048) as r:
        r.render_passes(3)
        check_images(cb, r, lambda g, m: r.grayscale_image(g, m), 1, lambda a: a)
        r.set_density_filter(*FILTER)
        with pytest.raises(cb.CudabrotError):  # a filtered renderer makes no colour image
            r.color_image((0, 0, 0))
        r.set_density_filter(0)
        assert r.color_image((0, 0, 0))[0].shape == (64, 64, 3)


def test_palette_renderer_smooths_a_colour_pixel_as_one_thing(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 64), cb.IterationControl(500, 20), device=0, n_threads=1000) as r:
        r.set_palette(plot.demo_table(500))
        r.render_passes(3)
        hist = r.read_histogram()
        t = cb.density_thresholds(*FILTER)
        assert hist.shape == (3, 64, 64)
        assert not np.array_equal(cb.density_filter(hist, t, 3), cb.density_filter(hist, t, 1))  # the group matters here
        check_images(cb, r, r.palette_image, 3, lambda a: a.transpose(2, 0, 1).reshape(3 * 64, 64))


def test_depth_renderer_filters_each_slice_on_its_own(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 64), cb.IterationControl(500, 20), device=0, n_threads=1000) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 4))
        r.render_passes(3)
        assert r.read_histogram().shape == (4, 64, 64)
        check_images(cb, r, r.depth_image, 1, lambda a: a.reshape(4 * 64, 64))


def test_channel_renderer_filters_each_plane_on_its_own(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 64), [(300, 20), (60, 10)], n_threads=2048) as r:
        r.render_passes(3)
        hist = r.read_histogram()
        assert hist.shape == (2, 64, 64)
        r.set_density_filter(*FILTER)
        for clip in (0.0, 2.0):
            r.set_white_clip(clip)
            for plane in (0, 1):
                want, want_max, want_scale = host_image(cb, hist[plane], 1, 2.2, clip)
                for mode in MODES:
                    got, mx, scale = r.grayscale_image(2.2, getattr(cb, mode), plane=plane)
                    assert (mx, scale) == (want_max, want_scale) and np.array_equal(got.astype(np.uint16), want), (clip, plane, mode)


# ---- the binary ----

LINE = "Density filter: radius 4, alpha 0.5, n0 2 (the values above carry 8 fraction bits)"


def test_cli_writes_one_file_in_every_tone_form_and_leaves_the_state_alone(cb, exe, tmp_path):  # noqa: F811
    common = ["-m", "300", "-w", "64", "-h", "64", "--passes", "2", "--stats"]
    flag = ["--density-filter", "4:0.5:2"]
    forms = {"auto": [], "lut": ["--tonemap", "lut"], "thresholds": ["--tonemap", "thresholds"], "host": ["--tonemap", "host"]}
    files = {k: [str(tmp_path / (k + e)) for e in (".pgm", ".bin", ".rng")] for k in list(forms) + ["plain"]}
    runs = {k: run(exe, *common, *flag, *more, "-o", files[k][0], "-s", files[k][1], "--rng-state", files[k][2])
            for k, more in forms.items()}
    runs["plain"] = run(exe, *common, "-o", files["plain"][0], "-s", files["plain"][1], "--rng-state", files["plain"][2])
    for k, r in runs.items():
        assert r.returncode == 0, r.stdout + r.stderr
    hist = read_state_file(files["plain"][1], 64, 64)
    filtered = cb.density_filter(hist, cb.density_thresholds(4, 0.5, 2))
    gray, mx, scale = cb.set_grayscale_pixels(filtered, 1.0)
    want = b"P5\n64 64\n65535\n" + gray.astype(">u2").tobytes()
    plain = open(files["plain"][0], "rb").read()
    assert plain != want and "Density filter" not in runs["plain"].stdout
    for k in forms:
        assert open(files[k][0], "rb").read() == want, k
        assert open(files[k][1], "rb").read() == open(files["plain"][1], "rb").read(), k   # the -s file
        assert open(files[k][2], "rb").read() == open(files["plain"][2], "rb").read(), k   # the generator states
        lines = runs[k].stdout.split("\n")
        at = lines.index(LINE)
        assert lines[at - 1] == "Max value: %d, scale: %f" % (mx, scale), k
        said = [line for line in runs[k].stderr.split("\n") if line.startswith('{"density_filter"')]
        assert len(said) == 1
        stats = json.loads(said[0])
        assert "samples" in json.loads(runs[k].stderr.strip().split("\n")[-1])  # the counters' line is as it was
        alpha = stats["density_filter"].pop("alpha")  # a hexfloat, as C's %a writes it
        assert alpha.startswith("0x") and float.fromhex(alpha) == 0.5
        assert stats["density_filter"] == {"radius": 4, "n0": 2, "thresholds": [32, 8, 3, 2]}
        assert cb.density_thresholds(4, float.fromhex(alpha), 2)[1:] == [32, 8, 3, 2]
    assert "density_filter" not in runs["plain"].stderr


def test_cli_palette_and_clip_on_filtered_counters(cb, exe, tmp_path):  # noqa: F811
    common = ["-m", "300", "-w", "64", "-h", "64", "--passes", "2", "--palette", "0:ff0000,150:00ff00,299:0000ff",
              "--density-filter", "4:0.5:2", "--white-clip", "2"]
    bodies, outs = {}, {}
    for k, more in {"device": [], "host": ["--tonemap", "host"]}.items():
        r = run(exe, *common, *more, "-o", str(tmp_path / (k + ".ppm")))
        assert r.returncode == 0, r.stdout + r.stderr
        bodies[k] = open(tmp_path / (k + ".ppm"), "rb").read()
        outs[k] = [line for line in r.stdout.split("\n") if line.startswith(("Max value", "Density filter", "White value"))]
    assert bodies["device"] == bodies["host"] and bodies["device"].startswith(b"P6\n64 64\n65535\n")
    assert outs["device"] == outs["host"] and len(outs["device"]) == 3 and outs["device"][1] == LINE
    assert [line.split(":")[0] for line in outs["device"]] == ["Max value", "Density filter", "White value"]


def test_cli_depth_planes_and_clip_on_filtered_counters(cb, exe, tmp_path):  # noqa: F811
    """The stacked shape -- N planes as N PGMs in one file -- is where the host loop's rows, groups of one plane and the
    byte swap meet: the same bytes and the same three lines from the device and from --tonemap host."""
    common = ["-m", "300", "-w", "64", "-h", "64", "--passes", "2", "--depth", "cr:-2:0.5:4", "--density-filter", "4:0.5:2",
              "--white-clip", "2"]
    bodies, outs = {}, {}
    for k, more in {"device": [], "host": ["--tonemap", "host"]}.items():
        r = run(exe, *common, *more, "-o", str(tmp_path / (k + ".pgm")))
        assert r.returncode == 0, r.stdout + r.stderr
        bodies[k] = open(tmp_path / (k + ".pgm"), "rb").read()
        outs[k] = [line for line in r.stdout.split("\n") if line.startswith(("Max value", "Density filter", "White value"))]
    header, plane = b"P5\n64 64\n65535\n", len(b"P5\n64 64\n65535\n") + 64 * 64 * 2
    assert bodies["device"] == bodies["host"] and len(bodies["device"]) == 4 * plane
    assert all(bodies["device"][s * plane:].startswith(header) for s in range(4))
    assert outs["device"] == outs["host"] and len(outs["device"]) == 3 and outs["device"][1] == LINE
    assert [line.split(":")[0] for line in outs["device"]] == ["Max value", "Density filter", "White value"]
