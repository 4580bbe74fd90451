"""The locally equalised image on the device (equalize_local.hip; include/cudabrot_amd.h, "Locally equalised image";
DESIGN.md 4.28): the tile-wise sweep equals the host's bins bit for bit and the blended image the host function's bytes --
on shapes chosen for the kernels' edges (a pixel per tile, odd widths and tile edges, one-dimensional grids, more blocks
than rows in a tile, pooled planes, a canvas the grid-stride loops wrap on, a base pointer that is not 16-byte aligned) and
on contents chosen for the count (key edges, crowded tiles on both sides of the LDS window, empty tiles) --, both entry
points refuse what they must with nothing written, and the renderer and the binary apply it to the array whose maximum they
take otherwise, its planes pooled."""

import ctypes as C

import numpy as np
import pytest

import equalize_reference as eq
import local_equalize_reference as leq
import plot_reference as plot
from conftest import read_state_file
from output_planted import FILL, guarded_output, on_device, read_guarded, source
from plot_harness import DEPTH_SHAPE, exe  # noqa: F401
from plot_harness import gpu_run as run

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
WINDOW = 8192  # equalize_local.hip's kLocalWindow: keys below it are counted in LDS, the others in global memory
MODES = ["CB_TONE_LUT", "CB_TONE_THRESHOLDS", "CB_TONE_AUTO"]
FILTER = (4, 0.5, 2)
CLIP = 1024  # the binary's default, 4


def test_the_window_named_here_is_the_code_s():
    assert source("equalize_local.hip")[1] == {"kLocalWindow": WINDOW}
    assert source("counter_sweep.h")[1]["kSweepBlocks"] == 1024  # 16 x 16 tiles: four blocks a tile


def on_both(cb, hist, tx, ty, settings=((CLIP, 2.2),), offset=0):
    """Device bins == host bins and, for every (clip_q, gamma), device bytes and numbers == the host function's."""
    import torch

    a = leq.planes_of(hist)
    planes, h, w = a.shape
    stream = torch.cuda.current_stream().cuda_stream
    base, view = on_device(a, offset)
    assert view.data_ptr() % 16 == (8 if offset % 2 else 0)
    got = cb.local_equalize_bins_device(view.data_ptr(), w, h, planes, tx, ty, stream=stream)
    want = cb.local_equalize_bins(a, tx, ty)
    assert got[1:] == want[1:], (got[1:], want[1:])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:8]
    for clip_q, gamma in settings:
        guard, out = guarded_output(a.size)
        numbers = cb.tone_map_device_local_equalized(view.data_ptr(), w, h, planes, tx, ty, clip_q, gamma, out.data_ptr(),
                                                     stream=stream)
        torch.cuda.synchronize()
        body = read_guarded(guard, a.size)
        gray, *host_numbers = cb.set_grayscale_pixels_local_equalized(a, tx, ty, clip_q, gamma)
        assert numbers[0] == host_numbers[0] and numbers[2:] == tuple(host_numbers[2:]), (clip_q, gamma)
        assert numbers[1] == host_numbers[1] or host_numbers[0] == 0
        assert body.tobytes() == gray.astype(">u2").tobytes(), (clip_q, gamma, np.flatnonzero(body != gray.reshape(-1))[:8])
    del base
    return got, want


BOTH = ((CLIP, 2.2), (0, 0.0))
# name -> (w, h, planes, tx, ty, offset of the base pointer in counters)
SHAPES = {
    "a_pixel_per_tile": (5, 3, 1, 5, 3, 0),           # dx = dy = 2 between any two centres
    "odd_width_odd_edges": (63, 37, 1, 4, 3, 0),      # a segment's alignment flips from row to row
    "odd_width_misaligned_base": (63, 37, 1, 4, 3, 1),
    "one_tile": (64, 48, 1, 1, 1, 0),
    "a_column_of_tiles": (64, 48, 1, 1, 4, 0),        # blends along y only
    "a_row_of_tiles": (64, 48, 1, 4, 1, 0),           # ... along x only
    "more_blocks_than_rows": (64, 48, 1, 16, 16, 0),  # tiles of 4 x 3, four blocks each
    "pooled_planes": (24, 32, 3, 2, 2, 0),
    "pooled_planes_misaligned": (25, 31, 3, 2, 3, 1),
    "a_segment_of_three_turns": (4099, 3, 1, 1, 1, 0),  # a block's share is one row of 2051 slots: its loop takes three turns
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_bins_and_bytes_equal_the_host_s_on_every_shape(cb, name):
    w, h, planes, tx, ty, offset = SHAPES[name]
    hist = eq.heavy(np.random.default_rng(w * h + planes), planes * h * w, 1 << 36).reshape(planes, h, w)
    got, _ = on_both(cb, hist, tx, ty, BOTH, offset)
    assert got[1] == int(np.count_nonzero(hist)) > 0 and got[2] == int(hist.max())


def test_a_canvas_of_odd_sides_in_the_most_tiles(cb):
    """1031 x 517 in 16 x 16 tiles of 64 or 65 by 32 or 33: 256 tiles of four blocks, keys on both sides of the window."""
    hist = eq.heavy(np.random.default_rng(41), 517 * 1031, 1 << 30).reshape(517, 1031)
    got, _ = on_both(cb, hist, 16, 16)
    assert got[2] > eq.lowest_count(WINDOW)


def test_a_canvas_the_map_s_grid_stride_loop_wraps_on(cb):
    """Four planes of 1031 x 517: more pixels than the 4096 blocks of the map take in one turn, two a lane."""
    hist = eq.heavy(np.random.default_rng(43), 4 * 517 * 1031, 1 << 30).reshape(4, 517, 1031)
    assert hist.size > 4096 * 256 * 2
    on_both(cb, hist, 3, 2)


def contents():
    """name -> (counters [h, w], tx, ty)."""
    below, at = eq.lowest_count(WINDOW - 1), eq.lowest_count(WINDOW)
    out = {"key_edges": (eq.key_edges(), 3, 3), "u64_max": (eq.cases()["u64_max"], 3, 1),
           "all_zero": (np.zeros((37, 63), dtype=np.uint64), 4, 3)}
    faint = np.arange(64 * 128, dtype=np.uint64).reshape(64, 128) % np.uint64(7)
    for name, value in (("below_window", below), ("at_window", at), ("far_above_window", (1 << 64) - 1)):
        hist = faint.copy()
        hist[:32, 64:] = value  # tile (1, 0) of 2 x 2: 64 x 32 counters of one key
        out["crowded_" + name] = (hist, 2, 2)
    side = faint.copy()
    side[32:, :64] = np.where(np.arange(64) % 2 == 0, below, at).astype(np.uint64)  # keys W - 1 and W, lane by lane
    out["window_edge_side_by_side"] = (side, 2, 2)
    lit_beside_empty = np.zeros((48, 64), dtype=np.uint64)
    lit_beside_empty[:, :17] = eq.heavy(np.random.default_rng(9), 48 * 17, 1 << 24).reshape(48, 17) + np.uint64(1)
    out["an_empty_tile_beside_a_lit_one"] = (lit_beside_empty, 4, 2)
    return out


CONTENTS = contents()


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_contents_made_to_break_the_count(cb, name):
    hist, tx, ty = CONTENTS[name]
    got, want = on_both(cb, hist, tx, ty, BOTH)
    if name.startswith("crowded"):
        value = int(hist[0, 64])
        assert int(got[0][1][eq.key(value)]) == 64 * 32 and np.count_nonzero(got[0][1]) == 1  # tile (1, 0): one bin
        assert (eq.key(value) < WINDOW) == (name == "crowded_below_window")
    if name == "window_edge_side_by_side":
        assert [int(got[0][2][WINDOW - 1]), int(got[0][2][WINDOW])] == [32 * 32] * 2
    if name == "all_zero":
        assert got[1:] == (0, 0) and not got[0].any()
    if name == "an_empty_tile_beside_a_lit_one":
        assert [int(got[0][t].sum()) > 0 for t in range(8)] == [True, True, False, False] * 2


def test_both_entry_points_refuse_bad_arguments_with_nothing_written(cb):
    import torch

    base, view = on_device(np.arange(1, 25, dtype=np.uint64))
    bins = np.full((4, eq.KEYS), 77, dtype=np.uint64)
    out = [C.c_uint64(7) for _ in range(3)]
    refs = [C.byref(v) for v in out]
    guard, gray = guarded_output(24)
    p, b, g = view.data_ptr(), bins.ctypes.data, gray.data_ptr()
    bad = [(None, 4, 3, 2, 2, 2), (p + 4, 4, 3, 2, 2, 2), (p, 0, 3, 2, 2, 2), (p, 4, -3, 2, 2, 2), (p, 4, 3, 0, 2, 2),
           (p, 4, 3, 2, 0, 2), (p, 4, 3, 2, 2, 0), (p, 4, 3, 2, 5, 2), (p, 4, 3, 2, 2, 4), (p, 4, 3, 2, 17, 2),
           (p, 1 << 20, 1 << 20, 2, 2, 2),                                          # more than 2^40 counters
           # 2^32 counters, admitted otherwise, but a tile row of 65536 over 65536 planes is 2^32: past a block's u32 bins
           # (decided before anything is read: the 24 counters here are all there is)
           (p, 1 << 16, 1, 1 << 16, 1, 1), (p, 1 << 17, 2, 1 << 16, 2, 2), (p, (1 << 16) + 1, 3, 1 << 16, 1, 3)]
    f = cb.lib.cb_local_equalize_bins_device
    for call in bad:
        assert f(*call, b, *refs[:2], None) == INVALID, call
    assert f(p, 4, 3, 2, 2, 2, None, *refs[:2], None) == INVALID
    assert f(p, 4, 3, 2, 2, 2, b, None, refs[1], None) == INVALID
    assert f(p, 4, 3, 2, 2, 2, b, refs[0], None, None) == INVALID
    e = cb.lib.cb_tone_map_device_local_equalized
    for call in bad:
        assert e(*call, CLIP, 1.0, g, None, None, *refs, None) == INVALID, call
    assert e(p, 4, 3, 2, 2, 2, CLIP, 1.0, None, None, None, *refs, None) == INVALID
    assert e(p, 4, 3, 2, 2, 2, CLIP, 1.0, g + 2, None, None, *refs, None) == INVALID     # the map stores two pixels at once
    for clip_q in (1, 255, 65537):
        assert e(p, 4, 3, 2, 2, 2, clip_q, 1.0, g, None, None, *refs, None) == INVALID, clip_q
    torch.cuda.synchronize()
    assert [v.value for v in out] == [7, 7, 7] and set(bins.reshape(-1).tolist()) == {77}
    assert (read_guarded(guard, 24).view(np.uint16) == FILL).all()
    # every output number of the image call is optional
    assert e(p, 4, 3, 2, 2, 2, CLIP, 1.0, g, None, None, None, None, None, None) == 0
    assert f(p, 4, 3, 2, 2, 2, b, *refs[:2], None) == 0 and [v.value for v in out[:2]] == [24, 24] and int(bins.sum()) == 24


# ---- the renderer: every image call takes the locally equalised map over the array it takes the maximum of ----

GRID = (4, 3)


def host_planes(cb, hist, group, gamma, filtered, clip_q=CLIP):
    """The host definition over a histogram [h, w] or [planes, h, w], its planes pooled -> (u16 [rows, w], max, scale,
    numbers)."""
    if filtered:
        hist = cb.density_filter(hist, cb.density_thresholds(*FILTER), group)
    gray, mx, scale, *numbers = cb.set_grayscale_pixels_local_equalized(hist, *GRID, clip_q, gamma)
    rows = hist.reshape(-1, hist.shape[-1])
    assert numbers[0] > 0 and (mx, scale) == cb.set_grayscale_pixels(rows, gamma)[1:]  # what the unflagged call returns
    return gray.reshape(rows.shape), mx, scale, tuple(numbers)


def check_images(cb, r, image, group, shape_out, pick=lambda planes: planes):
    """`image(gamma, mode)` of a rendered renderer `r`, locally equalised: plain and over the filtered counters, in every
    mode; `pick` takes the planes the image is made of out of the histogram read back."""
    hist = pick(r.read_histogram())
    plain, plain_max, plain_scale = image(2.2, 0)
    assert r.local_equalize == (0, 0, 0) and r.last_local_equalize() == (0, 0, 0)
    r.set_local_equalize(*GRID)
    assert r.local_equalize == (*GRID, CLIP) and r.last_local_equalize() == (0, 0, 0)
    for filtered in (False, True):
        r.set_density_filter(*(FILTER if filtered else (0,)))
        for gamma in (2.2, 0.0):
            want, want_max, want_scale, numbers = host_planes(cb, hist, group, gamma, filtered)
            for mode in MODES:
                got, mx, scale = image(gamma, getattr(cb, mode))
                assert (mx, scale) == (want_max, want_scale), (filtered, gamma, mode)
                assert np.array_equal(shape_out(got.astype(np.uint16)), want), (filtered, gamma, mode)
                assert r.last_local_equalize() == numbers
        if not filtered:
            assert (want_max, want_scale) == (plain_max, plain_scale)
    r.set_density_filter(0)
    # another clip is another image, and the numbers say what it moved
    r.set_local_equalize(*GRID, clip_q=0)
    want, _, _, numbers = host_planes(cb, hist, group, 2.2, False, clip_q=0)
    assert np.array_equal(shape_out(image(2.2, 0)[0].astype(np.uint16)), want) and r.last_local_equalize() == numbers
    assert numbers[2] == 0
    r.set_local_equalize(*GRID)
    # the mode is validated; a clip or equalisation beside it is refused and changes nothing; a grid the canvas cannot hold too
    with pytest.raises(cb.CudabrotError):
        image(2.2, 7)
    image(2.2, 0)
    before = r.last_local_equalize()
    assert cb.lib.cb_renderer_set_white_clip(r._h, 1.0) == INVALID and r.white_clip == 0.0
    assert cb.lib.cb_renderer_set_equalize(r._h, 1) == INVALID and not r.equalize
    for bad in ((17, 3, CLIP), (4, 0, CLIP), (4, 3, 255), (4, r.dims.h + 1, CLIP), (-1, 3, CLIP)):
        assert cb.lib.cb_renderer_set_local_equalize(r._h, *bad) == INVALID, bad
    assert r.local_equalize == (*GRID, CLIP) and r.last_local_equalize() == before
    assert cb.lib.cb_renderer_set_white_clip(r._h, 0.0) == 0 and cb.lib.cb_renderer_set_equalize(r._h, 0) == 0
    assert r.last_local_equalize() == before and r.last_white() == (0, 0, 0) and r.last_equalize() == (0, 0, 0)
    # an output setting: the histogram is what it was, and clearing it gives the unflagged bytes again
    assert np.array_equal(pick(r.read_histogram()), hist)
    r.set_local_equalize(0)
    assert r.local_equalize == (0, 0, 0) and r.last_local_equalize() == (0, 0, 0)
    again, again_max, again_scale = image(2.2, 0)
    assert (again_max, again_scale) == (plain_max, plain_scale) and again.tobytes() == plain.tobytes()
    # ... and local equalisation on a clipped or an equalised renderer is refused, the setting staying
    r.set_white_clip(1.0)
    clipped = image(2.2, 0)[0].tobytes()
    found = r.last_white()
    assert cb.lib.cb_renderer_set_local_equalize(r._h, *GRID, CLIP) == INVALID
    assert r.local_equalize == (0, 0, 0) and r.white_clip == 1.0 and r.last_white() == found
    assert image(2.2, 0)[0].tobytes() == clipped
    assert cb.lib.cb_renderer_set_local_equalize(r._h, 0, 0, 0) == 0 and r.white_clip == 1.0
    r.set_white_clip(0)
    r.set_equalize()
    assert cb.lib.cb_renderer_set_local_equalize(r._h, *GRID, CLIP) == INVALID and r.equalize and r.local_equalize == (0, 0, 0)
    r.set_equalize(False)


def test_grey_renderer(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 48), cb.IterationControl(300, 20), n_threads=2048) as r:
        r.render_passes(3)
        check_images(cb, r, lambda g, m: r.grayscale_image(g, m), 1, lambda a: a)
        r.set_local_equalize(*GRID)
        with pytest.raises(cb.CudabrotError):  # a locally equalised renderer makes no colour image
            r.color_image((0, 0, 0))
        r.set_local_equalize(0)
        assert r.color_image((0, 0, 0))[0].shape == (48, 64, 3)


def test_channel_renderer_equalises_each_plane_on_its_own(cb):
    with cb.Renderer(cb.FractalDimensions.make(64, 48), [(300, 20), (60, 10)], n_threads=2048) as r:
        r.render_passes(3)
        hist = r.read_histogram()
        assert hist.shape == (2, 48, 64)
        for plane in (0, 1):
            check_images(cb, r, lambda g, m, plane=plane: r.grayscale_image(g, m, plane=plane), 1, lambda a: a,
                         pick=lambda planes, plane=plane: planes[plane])
        assert host_planes(cb, hist[0], 1, 2.2, False)[3] != host_planes(cb, hist[1], 1, 2.2, False)[3]


def test_palette_renderer_pools_its_planes(cb):
    w, h = 64, 48
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(500, 20), device=0, n_threads=1000) as r:
        r.set_palette(plot.demo_table(500))
        r.render_passes(3)
        assert r.read_histogram().shape == (3, h, w)
        check_images(cb, r, r.palette_image, 3, lambda a: a.transpose(2, 0, 1).reshape(3 * h, w))


def test_depth_renderer_pools_its_slices(cb):
    w, h, max_iter, min_iter, threads, _ = DEPTH_SHAPE
    with cb.Renderer(cb.FractalDimensions.make(w, h), cb.IterationControl(max_iter, min_iter), device=0, n_threads=threads) as r:
        r.set_projection(cb.IDENTITY_PROJECTION)
        r.set_depth(("cr", -2.0, 0.5, 3))
        r.render_passes(3)
        hist = r.read_histogram()
        assert hist.shape == (3, h, w)
        check_images(cb, r, r.depth_image, 1, lambda a: a.reshape(3 * h, w))
        # pooled tiles are no slice's own, and no 4 x 9 grid over the stack either
        pooled = cb.set_grayscale_pixels_local_equalized(hist, *GRID, CLIP, 2.2)[0]
        assert any(not np.array_equal(pooled[s], cb.set_grayscale_pixels_local_equalized(hist[s], *GRID, CLIP, 2.2)[0])
                   for s in range(3))
        stacked = cb.set_grayscale_pixels_local_equalized(hist.reshape(3 * h, w), GRID[0], 3 * GRID[1], CLIP, 2.2)[0]
        assert not np.array_equal(pooled.reshape(3 * h, w), stacked)


def test_frames_renderer_pools_its_frames(cb):
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
SAID = "Locally equalized: %dx%d tiles, clip %d/256, %d lit pixels in %d lit tiles, %d counts moved"


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
    runs = cli_runs(exe, tmp_path, {k: ["--local-equalize", "4x3:2", "--tonemap", k] for k in ("lut", "thresholds", "host")})
    runs.update(cli_runs(exe, tmp_path, {"plain": [], "plain_host": ["--tonemap", "host"]}))
    hist = read_state_file(runs["lut"][2], 48, 64)
    gray, mx, scale, lit, lit_tiles, moved = cb.set_grayscale_pixels_local_equalized(hist, 4, 3, 512, 0.5)
    assert lit > 0 and lit_tiles > 1 and moved > 0
    for k in ("lut", "thresholds", "host"):
        r, image, state = runs[k]
        assert open(image, "rb").read() == HEADER + gray.astype(">u2").tobytes(), k
        assert np.array_equal(read_state_file(state, 48, 64), hist), k
        lines = r.stdout.split("\n")
        at = [i for i, said in enumerate(lines) if said.startswith("Locally equalized:")]
        assert len(at) == 1 and lines[at[0]] == SAID % (4, 3, 512, lit, lit_tiles, moved), r.stdout
        assert lines[at[0] - 1] == "Max value: %d, scale: %f" % (mx, scale), k              # what it is without the flag
        assert [s for s in r.stderr.split("\n") if "local_equalize" in s] == ['{"local_equalize": {"tiles": [4, 3], "clip_q": 512}}'], k
    # the run without the flag is what it was: the unflagged bytes, the same -s file, no line of the flag's
    plain_gray, plain_max, plain_scale = cb.set_grayscale_pixels(hist, 0.5)
    plain = open(runs["plain"][1], "rb").read()
    assert plain == open(runs["plain_host"][1], "rb").read() == HEADER + plain_gray.astype(">u2").tobytes()
    assert plain != open(runs["host"][1], "rb").read()
    assert open(runs["plain"][2], "rb").read() == open(runs["host"][2], "rb").read() == open(runs["lut"][2], "rb").read()
    for k in ("plain", "plain_host"):
        assert "equalized" not in runs[k][0].stdout and "equalize" not in runs[k][0].stderr
        assert "Max value: %d, scale: %f" % (plain_max, plain_scale) in runs[k][0].stdout.split("\n")

    def said(k):
        r, image, state = runs[k]
        lines = [s.replace(image, "FILE").replace(state, "STATE") for s in r.stdout.split("\n")]
        return [s for s in lines if " passes took " not in s and not s.startswith("Locally equalized:")]

    assert said("plain_host") == said("host") and len(said("host")) == len(runs["host"][0].stdout.split("\n")) - 2


def test_cli_equalizes_the_filtered_counters_of_a_stack_tile_by_tile(cb, exe, tmp_path):  # noqa: F811
    common = ["-m", "300", "-w", "64", "-h", "48", "--passes", "2", "--depth", "cr:-2:0.5:3", "--density-filter", "4:0.5:2",
              "--local-equalize", "4x3", "-g", "2.2"]
    bodies, outs = {}, {}
    for k, more in {"device": [], "host": ["--tonemap", "host"]}.items():
        r = run(exe, *common, *more, "-o", str(tmp_path / (k + ".pgm")), "-s", str(tmp_path / (k + ".bin")))
        assert r.returncode == 0, r.stdout + r.stderr
        bodies[k] = open(tmp_path / (k + ".pgm"), "rb").read()
        outs[k] = [line for line in r.stdout.split("\n") if line.startswith(("Max value", "Density filter", "Locally equalized"))]
    hist = read_state_file(str(tmp_path / "device.bin"), 48, 64, planes=3)
    filtered = cb.density_filter(hist, cb.density_thresholds(4, 0.5, 2))
    gray, mx, scale, lit, lit_tiles, moved = cb.set_grayscale_pixels_local_equalized(filtered, 4, 3, CLIP, 2.2)
    want = b"".join(HEADER + gray[s].astype(">u2").tobytes() for s in range(3))
    assert bodies["device"] == bodies["host"] == want
    assert outs["device"] == outs["host"] == [
        "Max value: %d, scale: %f" % (mx, scale),
        "Density filter: radius 4, alpha 0.5, n0 2 (the values above carry 8 fraction bits)",
        SAID % (4, 3, CLIP, lit, lit_tiles, moved)]
