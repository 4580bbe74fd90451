"""The oracle against the reference's OWN lines compiled for the host (oracle/_ref/libref_fma.so).

oracle/_ref is built by oracle/Makefile from the reference's source where it lies (build container) and
travels to the GPU box as a binary.  Where it is absent, every test compares with what those lines produced
when tests/golden/reference_lines.json was written (tests/golden/make_goldens.py, from the same library and
the same cases below): histograms by their digest, everything else value for value.
"""

import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_lines.json")


def golden(section):
    with open(GOLDEN) as f:
        return json.load(f)[section]


@pytest.fixture(scope="module")
def ref(oracle):
    """The reference's lines where they were built, else None (the tests then read reference_lines.json)."""
    return oracle.ref_library("fma")


def ref_render(ref, w, h, max_iter, min_iter, threads, passes, box, first=0, spt=50):
    hist = np.zeros((h, w), dtype=np.uint32)
    rc = ref.ref_draw(w, h, box[0], box[1], box[2], box[3], max_iter, min_iter, first, threads, passes, spt,
                      hist.ctypes.data)
    assert rc == 0
    return hist.astype(np.uint64)


def hist_digest(oracle, hist):
    return {"increments": int(hist.sum()), "max": int(hist.max()), "nonzero": int((hist > 0).sum()),
            "fnv1a64": "%016x" % oracle.fnv1a_pixels(hist)}


def sha256(data):
    return hashlib.sha256(data).hexdigest()


CONFIGS = [
    (256, 256, 100, 20, 20000, 1, (-2.0, 2.0, -2.0, 2.0), 0),
    (1000, 1000, 100, 20, 5000, 2, (-2.0, 2.0, -2.0, 2.0), 0),
    (200, 100, 100, 20, 20000, 1, (0.0, 1.0, 0.0, 0.5), 0),
    (4096, 4096, 2000, 20, 20000, 1, (-2.0, 2.0, -2.0, 2.0), 0),
    (4096, 4096, 20000, 20, 20000, 1, (-2.0, 2.0, -2.0, 2.0), 0),
    (2000, 1500, 2000, 20, 20000, 2, (-2.0, 2.0, -1.5, 1.5), 0),
    (333, 77, 500, 0, 3000, 2, (-1.7, 0.9, -0.3, 1.1), 0),
    (300, 300, 3000, 1000, 6000, 2, (-2.0, 2.0, -2.0, 2.0), 0),
    (256, 256, 400, 20, 4096, 2, (-2.0, 2.0, -2.0, 2.0), 262144),
    (256, 256, 400, 20, 4096, 1, (-2.0, 2.0, -2.0, 2.0), 7 * 262144),
    (64, 64, 0, 20, 500, 1, (-2.0, 2.0, -2.0, 2.0), 0),
    (64, 64, 50, 80, 500, 1, (-2.0, 2.0, -2.0, 2.0), 0),
]


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_histogram_equals_reference_lines(oracle, ref, i):
    w, h, mx, mn, t, p, box, first = CONFIGS[i]
    mine, _ = oracle.render(w, h, mx, mn, t, p, box, first_subsequence=first)
    if ref is not None:
        assert np.array_equal(mine, ref_render(ref, w, h, mx, mn, t, p, box, first))
    assert hist_digest(oracle, mine) == golden("histograms")[str(i)]


SHIP_CONFIGS = [
    (256, 256, 100, 20, 20000, 1, (-2.0, 2.0, -2.0, 2.0), 0),
    (400, 300, 2000, 20, 8000, 2, (-2.0, 2.0, -2.0, 1.0), 0),
    (333, 77, 500, 0, 3000, 2, (-1.9, 0.9, -1.3, 0.4), 4096),
]


def ship_id(c):
    return "%dx%d_m%d_c%d" % c[:4]


@pytest.mark.parametrize("cfg", SHIP_CONFIGS, ids=ship_id)
def test_burning_ship_histogram_equals_reference_lines(oracle, cfg):
    """RENDER_BURNING_SHIP (cudabrot.cu:15-17,327-330,353-356,397-399): the oracle's run-time switch
    against the reference's lines compiled with the define."""
    w, h, m, c, t, p, box, first = cfg
    got, _ = oracle.render(w, h, m, c, t, p, box, first_subsequence=first, burning_ship=True)
    ship = oracle.ref_library("ship_fma")
    if ship is not None:
        assert np.array_equal(got, ref_render(ship, w, h, m, c, t, p, box, first))
    assert hist_digest(oracle, got) == golden("burning_ship_histograms")[ship_id(cfg)]
    plain, _ = oracle.render(w, h, m, c, t, p, box, first_subsequence=first)
    assert not np.array_equal(got, plain)          # and the switch is off again afterwards


RNG_SUBSEQUENCES = (0, 1, 2, 63, 64, 19999, 262143, 262144, 2097151, (1 << 33) + 5)


def ref_rng_rows(ref):
    rows = []
    for s in RNG_SUBSEQUENCES:
        out = (C.c_uint32 * 64)()
        ref.ref_rng_u32(1337, s, 64, out)
        re, im = C.c_double(), C.c_double()
        ref.ref_first_sample(1337, s, C.byref(re), C.byref(im))
        rows.append({"subsequence": s, "u32": list(out), "first_sample": [re.value.hex(), im.value.hex()]})
    return rows


def test_rng_stream_equals_rocrand(oracle, ref):
    rows = ref_rng_rows(ref) if ref is not None else golden("rng")
    assert [r["subsequence"] for r in rows] == list(RNG_SUBSEQUENCES)
    for r in rows:
        s = r["subsequence"]
        assert r["u32"] == oracle.rng_u32(1337, s, 64), s
        assert tuple(float.fromhex(x) for x in r["first_sample"]) == oracle.first_sample(1337, s), s


def sample_points():
    rng = np.random.default_rng(7)
    pts = rng.uniform(-2.0, 2.0, size=(20000, 2))
    # points hugging the cardioid and the period-2 bulb, where a different contraction would flip the test
    th = rng.uniform(0, 2 * np.pi, size=4000)
    card = np.stack([0.5 * np.cos(th) - 0.25 * np.cos(2 * th), 0.5 * np.sin(th) - 0.25 * np.sin(2 * th)], axis=1)
    bulb = np.stack([-1.0 + 0.25 * np.cos(th), 0.25 * np.sin(th)], axis=1)
    eps = rng.uniform(-1e-15, 1e-15, size=(4000, 2))
    return np.concatenate([pts, card + eps, bulb + eps])


ITERATED_POINTS = 3000


def ref_point_functions(ref, pts):
    """The reference's set shortcut (one digit per point) and its escape index at max 300 of the first points."""
    return {"points_sha256": sha256(np.ascontiguousarray(pts, dtype="<f8").tobytes()),
            "in_set_shortcut": "".join(str(ref.ref_in_set_shortcut(re, im)) for re, im in pts),
            "iterate_mandelbrot_300": [ref.ref_iterate_mandelbrot(re, im, 300) for re, im in pts[:ITERATED_POINTS]]}


def test_point_functions_on_random_and_boundary_points(oracle, ref):
    pts = sample_points()
    theirs = ref_point_functions(ref, pts) if ref is not None else golden("point_functions")
    assert theirs["points_sha256"] == sha256(np.ascontiguousarray(pts, dtype="<f8").tobytes())
    for (re, im), code in zip(pts, theirs["in_set_shortcut"]):
        mine = (1 if oracle.lib.orc_in_main_cardioid(re, im) else 0) | (2 if oracle.lib.orc_in_order2_bulb(re, im) else 0)
        assert mine == int(code), (re, im)
    for (re, im), n in zip(pts[:ITERATED_POINTS], theirs["iterate_mandelbrot_300"]):
        assert oracle.lib.orc_iterate_mandelbrot(re, im, 300) == n, (re, im)
    assert len(theirs["in_set_shortcut"]) == len(pts) and len(theirs["iterate_mandelbrot_300"]) == ITERATED_POINTS


GAMMAS = [1.0, 2.2, 0.5, 0.0, -1.0]


def tonemap_hist(oracle):
    hist, _ = oracle.render(120, 90, 200, 20, 3000, 1, (-2.0, 1.0, -1.2, 1.2))
    return hist


def ref_tonemap(ref, hist, gamma, path):
    """The reference's tone map and PGM writer on `hist`: its gray pixels and the bytes of its file (it also prints
    its "Max value" line)."""
    h32 = hist.astype(np.uint32)
    rgray = np.zeros((90, 120), dtype=np.uint16)
    ref.ref_set_grayscale_pixels(h32.ctypes.data, 120, 90, gamma, rgray.ctypes.data)
    gray = rgray.copy()     # the writer swaps the buffer to big-endian in place
    ref.ref_save_image(os.fsencode(path), rgray.ctypes.data, 120, 90)
    with open(path, "rb") as f:
        return gray, f.read()


@pytest.mark.parametrize("gamma", GAMMAS)
def test_tonemap_and_pgm_equal_reference_lines(oracle, ref, tmp_path, gamma, capfd):
    hist = tonemap_hist(oracle)
    gray, mx, scale = oracle.set_grayscale_pixels(hist, gamma)
    line = "Max value: %d, scale: %f\n" % (mx, scale)   # cudabrot.cu:437
    if ref is not None:
        capfd.readouterr()
        rgray, pgm = ref_tonemap(ref, hist, gamma, str(tmp_path / "ref.pgm"))
        assert capfd.readouterr().out == line
        assert np.array_equal(gray, rgray)
        assert pgm == oracle.encode_pgm(gray)
    g = golden("tonemap")[repr(gamma)]
    assert g["stdout"] == line
    assert g["gray_sha256"] == sha256(np.ascontiguousarray(gray, dtype="<u2").tobytes())
    assert g["pgm_sha256"] == sha256(oracle.encode_pgm(gray))
