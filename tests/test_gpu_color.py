"""The colour stage on the device (include/cudabrot_amd.h, "Colour image"): cb_compose_color_device,
Renderer.color_image and `cudabrot --color` must give the bytes of the host restatement (cb_compose_color) and of the
numpy one (tests/color_reference.py) on the same tone-mapped planes."""

import os
import re

import numpy as np
import pytest

import color_reference as ref
from device_launches import gpu_run as run
from plot_harness import exe  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

T = 512 * 512  # the CLI always runs the reference's 512 x 512 threads


def _histograms(seed, h, w, big_plane=None):
    """Three Buddhabrot-like planes: mostly zeros, a heavy tail; plane `big_plane` has a max above 2^24."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(3):
        a = (rng.pareto(1.1, size=(h, w)) * (4 + 40 * j)).astype(np.uint64)
        a[rng.random((h, w)) < 0.85] = 0
        a = np.minimum(a, np.uint64(3_000_000))
        if j == big_plane:
            a = a * np.uint64(9)
            a[rng.integers(0, h), rng.integers(0, w)] = (1 << 24) + 12345
        out.append(a)
    return out


def _device_compose(cb, hists, gamma, mode, compose, stretch, hue):
    import torch

    h, w = hists[0].shape
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(a.view(np.int64).reshape(-1)).to(dev) for a in hists]
    d_rgb = torch.zeros(3 * h * w, dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    levels = cb.compose_color_device([t.data_ptr() for t in d], w, h, gamma, d_rgb.data_ptr(), mode=mode,
                                     compose=compose, stretch=stretch, hue_shift=hue, stream=stream)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy().view(">u2").reshape(h, w, 3), levels


PARAMS = [("rgb", (2.0, 1.0), 0.0), ("hsl", (2.0, 1.0), 0.3), ("hsl", (0.0, 0.0), -1.7), ("rgb", (5.0, 10.0), 2.0)]
# (h, w, the plane whose max is above 2^24): every parameter set on the small canvases, two on the large one
CASES = [(1, 1, None, p) for p in PARAMS] + [(77, 333, 1, p) for p in PARAMS] + [(3001, 4099, 2, p) for p in PARAMS[:2]]


@pytest.mark.parametrize("mode_name", ["CB_TONE_LUT", "CB_TONE_THRESHOLDS"])
@pytest.mark.parametrize("h,w,big,params", CASES)
def test_device_compose_equals_host_compose(cb, mode_name, h, w, big, params):
    compose, stretch, hue = params
    hists = _histograms(h * 7 + w, h, w, big)
    gamma = 2.2
    rgb, levels = _device_compose(cb, hists, gamma, getattr(cb, mode_name), compose, stretch, hue)
    grays = [cb.set_grayscale_pixels(a, gamma)[0] for a in hists]
    want, want_levels = cb.compose_color(grays, compose=compose, stretch=stretch, hue_shift=hue)
    assert levels == want_levels
    assert rgb.tobytes() == want.tobytes()
    if h * w < 100_000:
        np_rgb, np_levels = ref.compose(grays, compose, stretch[0], stretch[1], hue)
        assert np_levels == levels and rgb.tobytes() == np_rgb.astype(">u2").tobytes()


def test_device_compose_of_flat_planes(cb):
    """All-zero and constant planes (white <= black) and one of a single value above 2^24."""
    z = np.zeros((31, 17), dtype=np.uint64)
    c = np.full((31, 17), 5, dtype=np.uint64)
    big = np.full((31, 17), (1 << 30) + 1, dtype=np.uint64)
    for mode in (cb.CB_TONE_LUT, cb.CB_TONE_THRESHOLDS):
        rgb, levels = _device_compose(cb, [z, c, big], 1.0, mode, "rgb", (2.0, 1.0), 0.0)
        grays = [cb.set_grayscale_pixels(a, 1.0)[0] for a in (z, c, big)]
        want, want_levels = cb.compose_color(grays, "rgb")
        assert levels == want_levels and rgb.tobytes() == want.tobytes()


def test_renderer_color_image_equals_host_compose_of_its_planes(cb):
    """A three-window channel renderer, two calls of passes (carry, then the drain the read does): the device colour
    image equals the host compose of the renderer's own device tone maps, for any order of the planes."""
    dims = cb.FractalDimensions.make(301, 203)
    with cb.Renderer(dims, [(100, 20), (400, 100), (1500, 400)], n_threads=16384) as r:
        r.render_passes(3)
        r.render_passes(2)
        grays = [r.grayscale_image(2.2, plane=j)[0].astype(np.uint16) for j in range(3)]
        for planes, compose, hue in (((0, 1, 2), "rgb", 0.0), ((2, 0, 1), "hsl", 0.3)):
            rgb, levels = r.color_image(planes=planes, gamma=2.2, compose=compose, hue_shift=hue)
            want, want_levels = cb.compose_color([grays[j] for j in planes], compose=compose, hue_shift=hue)
            assert levels == want_levels
            assert rgb.tobytes() == want.tobytes()
        with pytest.raises(cb.CudabrotError):
            r.color_image(planes=(0, 1, 3))
        assert r.read_counters().status == 0


# ---- the binary ----

WINDOWS = [(100, 20), (400, 100), (1500, 400)]


def _color_run(exe, tmp_path, tag, *extra, color=True, env=None):
    pgms = [str(tmp_path / ("%s_c%d.pgm" % (tag, j))) for j in range(3)]
    ppm = str(tmp_path / ("%s.ppm" % tag))
    args = []
    for (m, c), o in zip(WINDOWS, pgms):
        args += ["--channel", "%d:%d:%s" % (m, c, o)]
    if color:
        args += ["--color", ppm, "--compose", "hsl", "--hue-shift", "0.3"]
    r = run(exe, "--passes", "2", "-w", "300", "-h", "200", "-g", "2.2", *args, *extra, env=env)
    assert r.returncode == 0, r.stdout
    return r, pgms, ppm


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_color_flag_composes_the_oracle_planes(exe, oracle, tmp_path):
    """--channel x3 --color: the PPM equals the numpy compose of the oracle's grays of the three windows; the PGMs
    are those of a run without --color; --tonemap host gives the same PPM bytes."""
    r, pgms, ppm = _color_run(exe, tmp_path, "dev")
    grays = []
    for m, c in WINDOWS:
        hist, _ = oracle.render(300, 200, m, c, T, 2, omp_threads=0)
        grays.append(oracle.set_grayscale_pixels(hist, 2.2)[0])
    want, levels = ref.compose(grays, "hsl", 2.0, 1.0, 0.3)
    assert _read(ppm) == ref.ppm_bytes(want)
    line = "Color levels: black %d %d %d, white %d %d %d" % tuple([b for b, _ in levels] + [w for _, w in levels])
    assert line in r.stdout
    tail = r.stdout[r.stdout.index(line):]
    assert tail == "%s\nSaving color image.\nDone! Color image saved: %s\n" % (line, ppm)

    _, plain_pgms, _ = _color_run(exe, tmp_path, "plain", color=False)
    for a, b in zip(pgms, plain_pgms):
        assert _read(a) == _read(b)

    rh, host_pgms, host_ppm = _color_run(exe, tmp_path, "host", "--tonemap", "host")
    assert _read(host_ppm) == _read(ppm)
    assert line in rh.stdout
    for a, b in zip(pgms, host_pgms):
        assert _read(a) == _read(b)


def test_color_flag_with_gpus_composes_the_reduced_planes(exe, tmp_path):
    """--gpus 2 (both ranks on device 0): the colour image is composed from rank 0's planes after the reduce, i.e.
    it is the compose of the PGMs the same run writes."""
    env = dict(os.environ, CUDABROT_AMD_FAKE_GPUS="1")
    r, pgms, ppm = _color_run(exe, tmp_path, "multi", "--gpus", "2", "--color-stretch", "0.5:0.25", env=env)
    assert re.search(r"^4 Buddhabrot passes took", r.stdout, re.M)
    grays = []
    for p in pgms:
        data = _read(p)
        assert data.startswith(b"P5\n300 200\n65535\n")
        grays.append(np.frombuffer(data[len(b"P5\n300 200\n65535\n"):], dtype=">u2").reshape(200, 300).astype(np.uint16))
    want, _ = ref.compose(grays, "hsl", 0.5, 0.25, 0.3)
    assert _read(ppm) == ref.ppm_bytes(want)


def test_color_write_failure_is_reported_and_the_run_still_succeeds(exe, tmp_path):
    bad = str(tmp_path / "no_such_dir" / "c.ppm")
    pgms = [str(tmp_path / ("f%d.pgm" % j)) for j in range(3)]
    args = []
    for (m, c), o in zip(WINDOWS, pgms):
        args += ["--channel", "%d:%d:%s" % (m, c, o)]
    r = run(exe, "--passes", "1", "-w", "64", "-h", "48", *args, "--color", bad)
    assert r.returncode == 0, r.stdout
    assert r.stdout.endswith("Saving color image.\nFailed opening output image.\nDone! Color image saved: %s\n" % bad)
