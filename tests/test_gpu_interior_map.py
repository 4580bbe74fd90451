"""The interior map (tools/interior_map.c; DrawArgs::interior_map): cells of the c-plane whose samples provably never
escape under the reference's iteration.  draw_wide_kernel's MID stage retires a sample of a marked cell as
never-escaping instead of iterating it until its fp64 orbit repeats bit for bit (~2000 iterations each).

The proof is the tool's (cell by cell); here the product is held to it the way VERDICT r02 #5 asks: identical histograms
and counters with the map, without it (CUDABROT_AMD_NO_INTERIOR_MAP=1, a test knob) and against the kernel that
iterates EVERY sample to max_iter like the reference (CB_KERNEL_FULL_ITERATE) -- over 10^10 samples of the headline
configuration and on windows made of interior; any sample of a marked cell that escaped would also raise
cb_counters.status (CB_STATUS_INTERIOR_MAP)."""

import numpy as np
import pytest

from device_launches import SAME, SQUARE, assert_same, renderer_render

pytestmark = pytest.mark.gpu


def built_level():
    """The level of the map kept in the tree (its header), which `make` embeds in the library."""
    import gzip
    import os
    import struct

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudabrot_amd", "interior_map.bin.gz")
    magic, level, _, _ = struct.unpack("<4I", gzip.open(path, "rb").read(16))
    assert magic == 0x4D494243
    return level


WIDE = 2


def render(cb, w, h, max_iter, threads, passes, box=SQUARE, variant=None):
    return renderer_render(cb, w, h, max_iter, 20, threads, passes, box=box, variant=variant)


def test_the_map_is_built_loaded_and_used(cb, oracle, monkeypatch):
    """`make` embeds the kept map in the library (level 12, proven nine levels of quarters deep); the wide kernel uses it and skips more iterations
    than the periodicity check alone -- with the oracle's histogram and counters."""
    args = (512, 512, 2000, 8192, 8)
    with_map = render(cb, *args)
    assert with_map[2] == WIDE and with_map[3] == built_level() >= 10, "no interior map in use"
    monkeypatch.setenv("CUDABROT_AMD_NO_INTERIOR_MAP", "1")
    without = render(cb, *args)
    assert without[2] == WIDE and without[3] == 0
    assert_same(with_map, without)
    assert with_map[1]["skipped_steps"] > without[1]["skipped_steps"] > 0
    ref = oracle.render(512, 512, 2000, 20, 8192, 8, omp_threads=0)
    assert np.array_equal(with_map[0], ref[0])
    for k in SAME:
        assert with_map[1][k] == ref[1][k], (k, with_map[1][k], ref[1][k])


def test_the_map_is_embedded_and_another_one_must_be_one_to_the_byte(cb, tmp_path):
    """VERDICT r03 #2a / ADVICE r03: the map decides results, so there is no file to find, lose or swap -- the library
    carries it (maps.S; `make` has checked its sha256 against the digest in the tree).  The one way to hand it another
    (CUDABROT_AMD_INTERIOR_MAP behind CUDABROT_AMD_DEBUG=1, a test knob; read once per device and process, hence the
    subprocesses) takes a map of exactly the right header AND length, and anything else -- no such file, not a map, a
    map one byte too long -- is an ERROR of the draw call, never a silent run without or with half a map.  Without any
    map (CUDABROT_AMD_NO_INTERIOR_MAP=1) the results are the same and more iterations are made."""
    import gzip
    import json
    import os
    import subprocess
    import sys

    prog = (
        "import json, numpy as np, cudabrot_amd as cb\n"
        "dims = cb.FractalDimensions.make(256, 256)\n"
        "try:\n"
        "    with cb.Renderer(dims, cb.IterationControl(1000, 20), n_threads=4096) as r:\n"
        "        r.render_passes(4)\n"
        "        h = r.read_histogram(); c = r.read_counters().as_dict()\n"
        "except cb.CudabrotError as e:\n"
        "    print(json.dumps({'error': e.code})); raise SystemExit(0)\n"
        "print(json.dumps({'level': cb.lib.cb_debug_interior_map_level(), 'sum': int(h.sum()), 'crc': int(np.bitwise_xor.reduce(h.ravel() * np.arange(1, h.size + 1, dtype=np.uint64))),"
        " 'never': c['never_escaped'], 'skipped': c['skipped_steps'], 'iterate': c['iterate_steps'], 'status': c['status']}))\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = gzip.open(os.path.join(root, "cudabrot_amd", "interior_map.bin.gz"), "rb").read()
    good = tmp_path / "copy_of_the_kept_map.bin"
    good.write_bytes(raw)
    bad = tmp_path / "not_a_map.bin"
    bad.write_bytes(b"CBIM" + bytes(100))
    long_ = tmp_path / "one_byte_too_long.bin"
    long_.write_bytes(raw + b"\0")
    short = tmp_path / "truncated.bin"
    short.write_bytes(raw[: len(raw) // 2])

    def run(**knobs):
        env = dict(os.environ, CUDABROT_AMD_DEBUG="1", **{k: str(v) for k, v in knobs.items()})
        out = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, check=True)
        return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr

    with_map, _ = run()
    assert with_map["level"] == built_level() and with_map["status"] == 0
    other, _ = run(CUDABROT_AMD_INTERIOR_MAP=good)
    assert other == with_map
    for path in (tmp_path / "no_such_file.bin", bad, long_, short):
        refused, err = run(CUDABROT_AMD_INTERIOR_MAP=path)
        assert "error" in refused and refused["error"] != 0, (path, refused)
        assert "refused" in err, err
    without, _ = run(CUDABROT_AMD_NO_INTERIOR_MAP=1)
    assert without["level"] == 0 and without["status"] == 0
    for k in ("sum", "crc", "never", "iterate"):
        assert without[k] == with_map[k], k
    assert without["skipped"] < with_map["skipped"]


def test_ten_billion_samples_against_full_iteration(cb):
    """C3 (4096^2, max_iter 20000, 262144 subsequences), 768 passes = 1.0e10 samples: the product against
    CB_KERNEL_FULL_ITERATE, which retires nothing early."""
    args = (4096, 4096, 20000, 262144, 768)
    product = render(cb, *args)
    assert product[2] == WIDE and product[3] == built_level()
    assert product[1]["samples"] >= 10 ** 10
    full = render(cb, *args, variant=cb.CB_KERNEL_FULL_ITERATE)
    assert full[3] == 0 and full[1]["skipped_steps"] == 0
    assert_same(product, full)
    assert product[1]["skipped_steps"] > 0.8 * product[1]["iterate_steps"]


WINDOWS = [
    (-0.25, 0.0, 0.55, 0.95),      # the period-3 bulb (upper)
    (-0.25, 0.0, -0.95, -0.55),    # ... and its mirror image: the map holds |im| only
    (-1.45, -1.15, -0.15, 0.15),   # the period-4 bulb on the real axis, both signs of im in one window
    (-1.80, -1.72, -0.04, 0.04),   # the period-3 cardioid of the antenna
    (0.2, 0.6, 0.3, 0.7),          # the right-hand edge of the map's columns (re = 0.5) inside the window
    (-0.6, 0.1, 0.9, 1.4),         # the upper edge of its rows (|im| = 1.25)
]


@pytest.mark.parametrize("box", WINDOWS, ids=["bulb3", "bulb3_mirror", "bulb4", "mini_cardioid", "re_edge", "im_edge"])
def test_windows_made_of_interior(cb, box):
    """Sampling windows are [-2,2]^2 in the reference; the map is consulted for c wherever the sample falls, so the
    interior is reached through the default sampling box.  What these windows vary is where the PIXELS are -- the
    samples are the same; the test is that nothing depends on it.  (The 10^10-sample test above is the one that
    sweeps the map's cells.)"""
    args = (384, 384, 3000, 16384, 6)
    product = render(cb, *args, box=box)
    assert product[2] == WIDE and product[3] == built_level()
    full = render(cb, *args, box=box, variant=cb.CB_KERNEL_FULL_ITERATE)
    assert_same(product, full)


def marked_cells_and_depths():
    """The marked cells of the kept map (their indices) and, if the tree has them, the depth each proof needed
    (cudabrot_amd/interior_map.depths.gz: `make verify-interior-map`)."""
    import gzip
    import os
    import struct

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = gzip.open(os.path.join(root, "cudabrot_amd", "interior_map.bin.gz"), "rb").read()
    magic, level, cols, rows = struct.unpack("<4I", raw[:16])
    marked = np.flatnonzero(np.unpackbits(np.frombuffer(raw, dtype=np.uint8, offset=16), bitorder="little"))
    depths = None
    side = os.path.join(root, "cudabrot_amd", "interior_map.depths.gz")
    if os.path.exists(side):
        d = gzip.open(side, "rb").read()
        m2, l2, n2, _ = struct.unpack("<4I", d[:16])
        assert m2 == 0x44494243 and l2 == level and n2 == marked.size
        depths = np.frombuffer(d, dtype=np.uint8, offset=16)
    return level, cols, rows, marked, depths


def test_the_reference_s_own_function_never_escapes_inside_marked_cells(cb, oracle):
    """VERDICT r03 #2d: the map's claim, put to the reference's OWN IterateMandelbrot (cudabrot.cu:319-340, compiled for
    gfx950 with its own flags: oracle/_ref/libref_probe.so) on the MI355X -- 10^8 points drawn inside marked cells, half
    of them inside the cells whose proof went deepest (the boundary layer, where a wrong bit would be), at max_iter 20000
    and 60000: every one must come back as max_iter (never escaped), which is what the kernel books for a marked sample
    without iterating it (cudabrot.cu:407)."""
    import ctypes as C
    import os

    path = os.path.join(oracle.REF_DIR, "libref_probe.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref/libref_probe.so not built (make -C oracle ref, needs /root/reference)")
    probe = C.CDLL(path)
    probe.ref_probe_points.restype = C.c_int
    probe.ref_probe_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    level, cols, rows, marked, depths = marked_cells_and_depths()
    deep = marked if depths is None else marked[depths >= max(1, int(np.percentile(depths, 90)))]
    s = 2.0 ** -level
    rng = np.random.default_rng(2026)
    batch, total = 5_000_000, 0
    for max_iter, batches in ((20000, 16), (60000, 4)):
        for _ in range(batches):
            cells = np.concatenate([rng.choice(marked, batch // 2), rng.choice(deep, batch - batch // 2)])
            re = -2.0 + (cells % cols + rng.random(batch)) * s
            im = (cells // cols + rng.random(batch)) * s * rng.choice(np.array([-1.0, 1.0]), batch)
            re, im = np.ascontiguousarray(re), np.ascontiguousarray(im)
            k = np.empty(batch, dtype=np.int32)
            sc = np.empty(batch, dtype=np.int32)
            rc = probe.ref_probe_points(re.ctypes.data, im.ctypes.data, batch, max_iter, k.ctypes.data, sc.ctypes.data)
            assert rc == 0, "HIP error %d in the probe" % rc
            bad = np.flatnonzero(k != max_iter)
            assert bad.size == 0, "the reference escapes at %s inside a marked cell: c = %r %r" % (
                k[bad[:3]], re[bad[:3]], im[bad[:3]])
            total += batch
    assert total >= 100_000_000
