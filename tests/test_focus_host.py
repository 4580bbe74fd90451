"""The focused render (include/cudabrot_amd.h, "Focused render") without a GPU: the host side of the cell list against a
numpy dilation, the mask's size, and the CPU restatement (tests/focus_reference.c) pinned to the oracle and to the
six-draw mapping's edges."""

import ctypes as C
import os

import numpy as np
import pytest

import focus_reference as focus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return focus.load(tmp_path_factory.mktemp("focus_ref"))


def omp_threads():
    v = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    return int(v) if v.isdigit() and int(v) > 0 else 16


def pack(grid):
    """bool [n, n] -> the mask's u32 words: bit (index & 31) of word (index >> 5), index = row * n + col."""
    return np.packbits(grid.reshape(-1), bitorder="little").view("<u4").astype(np.uint32)


def numpy_cells(grid, d):
    """Chebyshev dilation by d, clipped at the edge (a box is a row window followed by a column window), then the set
    cells in ascending order."""
    n = grid.shape[0]
    out = grid.copy()
    for axis in (0, 1):
        src = out
        out = src.copy()
        for s in range(1, min(d, n - 1) + 1):
            lo = [slice(None)] * 2
            hi = [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, n - s), slice(s, n)
            out[tuple(lo)] |= src[tuple(hi)]
            out[tuple(hi)] |= src[tuple(lo)]
    return np.flatnonzero(out.reshape(-1)).astype(np.uint32)


def planted(level, kind):
    n = 4 << level
    g = np.zeros((n, n), dtype=bool)
    rng = np.random.default_rng(1000 * level + len(kind))
    if kind == "empty":
        pass
    elif kind == "full":
        g[:] = True
    elif kind == "sparse":
        g[rng.integers(0, n, 40), rng.integers(0, n, 40)] = True
    elif kind == "dense":
        g = rng.random((n, n)) < 0.3
    elif kind == "corners":
        g[0, 0] = g[0, n - 1] = g[n - 1, 0] = g[n - 1, n - 1] = True
    elif kind == "edges":
        g[0, n // 3] = g[n - 1, n // 2] = g[n // 5, 0] = g[n // 2, n - 1] = True
    elif kind == "one":
        g[n // 2 + 1, n // 4 + 3] = True
    return g


@pytest.mark.parametrize("dilate", [0, 1, 3])
@pytest.mark.parametrize("kind", ["empty", "full", "sparse", "dense", "corners", "edges", "one"])
@pytest.mark.parametrize("level", [4, 8, 10])
def test_focus_cells_equals_a_numpy_dilation(cb, ref, level, kind, dilate):
    grid = planted(level, kind)
    want = numpy_cells(grid, dilate)
    got = cb.focus_cells(level, pack(grid), dilate)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    n = 4 << level
    if kind == "empty":
        assert got.size == 0
    if kind == "full":
        assert got.size == n * n
    if kind == "one":
        assert got.size == (2 * dilate + 1) ** 2
    if kind == "corners":  # clipped at the grid's edge: a quarter of each box and its two half edges
        assert got.size == 4 * (dilate + 1) ** 2
    if level < 10 or kind in ("sparse", "edges"):  # the restatement marks box by box: not for 16 Mi boxes
        assert np.array_equal(focus.cells(ref, level, pack(grid), dilate), want)


def test_focus_cells_with_a_dilation_wider_than_the_grid(cb):
    grid = planted(4, "one")
    assert np.array_equal(cb.focus_cells(4, pack(grid), 64), np.arange(64 * 64, dtype=np.uint32))
    assert np.array_equal(cb.focus_cells(4, pack(grid), 10 ** 6), np.arange(64 * 64, dtype=np.uint32))


def test_focus_cells_refuses_bad_arguments(cb):
    mask = np.zeros(focus.mask_words(4), dtype=np.uint32)
    n = C.c_uint32(7)
    for level, ptr, dilate, count in [(3, mask.ctypes.data, 1, C.byref(n)), (11, mask.ctypes.data, 1, C.byref(n)),
                                      (4, None, 1, C.byref(n)), (4, mask.ctypes.data, -1, C.byref(n)),
                                      (4, mask.ctypes.data, 1, None)]:
        assert cb.lib.cb_focus_cells(level, ptr, dilate, None, count) == 1  # hipErrorInvalidValue
    assert n.value == 7
    assert cb.lib.cb_focus_cells(4, mask.ctypes.data, 1, None, C.byref(n)) == 0 and n.value == 0


def test_focus_mask_bytes(cb):
    assert [cb.focus_mask_bytes(level) for level in (3, 4, 8, 10, 11)] == [0, 512, 128 * 1024, 2 * 1024 * 1024, 0]
    for level in range(cb.CB_FOCUS_MIN_LEVEL, cb.CB_FOCUS_MAX_LEVEL + 1):
        assert cb.focus_mask_bytes(level) == 4 * focus.mask_words(level) == (4 << level) ** 2 // 8


def test_focus_names_in_header_and_package(cb):
    import re

    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert int(re.search(r"#define CB_ERROR_FOCUS_EMPTY (\d+)", text).group(1)) == cb.CB_ERROR_FOCUS_EMPTY == 100002
    assert (cb.CB_FOCUS_MIN_LEVEL, cb.CB_FOCUS_MAX_LEVEL) == (4, 10)
    assert b"probe" in cb.lib.cb_error_string(cb.CB_ERROR_FOCUS_EMPTY)
    for name in ("focus_cells", "focus_mask_bytes", "focus_probe", "draw_buddhabrot_focus", "CB_ERROR_FOCUS_EMPTY"):
        assert name in cb.__all__
    assert hasattr(cb.Renderer, "set_focus") and hasattr(cb.Renderer, "focus_cells")


@pytest.mark.parametrize(
    "w,h,box,max_iter,min_iter,threads,ship",
    [
        (256, 256, (-2.0, 2.0, -2.0, 2.0), 500, 20, 4096, False),
        (300, 200, (-1.9, -0.7, -0.45, 0.35), 1000, 20, 4000, False),
        (256, 256, (-2.0, 2.0, -2.0, 2.0), 300, 5, 1337, True),
        (64, 64, focus.BOXES["body"], 500, 20, 4096, False),
    ],
    ids=["square", "ragged_zoom", "ship", "crop"],
)
def test_restatement_with_the_uniform_source_equals_the_oracle(ref, oracle, w, h, box, max_iter, min_iter, threads, ship):
    """Pins the restatement itself: without a cell list it is a normal render."""
    hist, cnt = focus.draw(ref, w, h, max_iter, min_iter, threads, [50, 50], box=box, ship=ship)
    par, cp = focus.draw(ref, w, h, max_iter, min_iter, threads, [50, 50], box=box, ship=ship, omp_threads=omp_threads())
    want, wc = oracle.render(w, h, max_iter, min_iter, threads, 2, box=box, burning_ship=ship)
    assert np.array_equal(hist, want) and np.array_equal(par, want)
    assert cnt == wc == cp
    assert cnt["samples"] == threads * 100 and int(hist.sum()) == cnt["increments"] > 0


def test_six_draw_mapping_on_planted_generator_outputs(ref):
    top = 2 ** 32 - 1
    for level in (4, 8, 10):
        n = 4 << level
        cells = np.array([0, 5, n + 1, (n // 2) * n + n // 2, n * n - 1], dtype=np.uint32)  # the fourth: corner (0, 0)
        side = 2.0 ** -level
        # a = b = 0 picks the first entry, a = b = 2^32 - 1 the last, whatever n_cells
        for count in (1, 2, 5):
            assert focus.mapping(ref, level, cells[:count], 0, 0, 0, 0, 0, 0)[0] == 0
            assert focus.mapping(ref, level, cells[:count], top, top, 0, 0, 0, 0)[0] == count - 1
        # j = floor(u * n_cells) for u = (a << 32 | b) / 2^64
        assert focus.mapping(ref, level, cells, 0x33333333, 0x33333333, 0, 0, 0, 0)[0] == 0  # 5 u just below 1
        assert focus.mapping(ref, level, cells, 0x33333333, 0x33333334, 0, 0, 0, 0)[0] == 1  # 5 u just above 1
        assert focus.mapping(ref, level, cells, 0x80000000, 0, 0, 0, 0, 0)[0] == 2           # u = 1/2
        # in the cell whose corner is (0, 0) the coordinates ARE the offsets: v = 0 gives the smallest, 2^-53-L, and
        # v = 2^53 - 1 (the first draw all ones, the second's upper 21 bits) exactly the cell's side
        j, re, im = focus.mapping(ref, level, cells, 0xA0000000, 0, 0, 0, top, top)  # u = 5/8
        assert j == 3 and re == 2.0 ** (-53 - level) and im == side
        j, re, im = focus.mapping(ref, level, cells, 0xA0000000, 0, top, top & ~0x7FF, 0, 0x7FF)
        assert j == 3 and re == side and im == 2.0 ** (-53 - level)  # the low 11 bits of the second draw are dropped
        # elsewhere: ONE rounded addition of the exact corner and the exact offset (python's + is that addition)
        lo = -2.0 + side
        _, re, im = focus.mapping(ref, level, cells, 0x80000000, 0, 0, 0, top, top)  # cell n + 1
        assert re == lo + 2.0 ** (-53 - level) and im == lo + side  # im: on the cell's upper edge, as defined
        _, re, im = focus.mapping(ref, level, cells, 0x80000000, 0, 12345, 0x00ABC000, 0xDEADBEEF, 0x12345678)
        vx, vy = 12345 | ((0x00ABC000 >> 11) << 32), 0xDEADBEEF | ((0x12345678 >> 11) << 32)
        assert re == lo + float(vx + 1) * 2.0 ** (-53 - level) and im == lo + float(vy + 1) * 2.0 ** (-53 - level)
        # the last cell's upper edge is 2.0 itself
        _, re, im = focus.mapping(ref, level, cells, top, top, top, top, top, top)
        assert (re, im) == (2.0, 2.0)
        _, re, im = focus.mapping(ref, level, cells, 0, 0, 0, 0, 0, 0)
        assert re == im == -2.0 + 2.0 ** (-53 - level)


def test_the_focused_stream_consumes_six_draws_per_sample(ref, oracle):
    """A thread that draws s focused samples leaves its generator where 6 s plain outputs leave it."""
    threads, samples = 7, 11
    cells = np.array([1000, 2000, 30000], dtype=np.uint32)
    st = oracle.init_states(1337, 0, threads)
    focus.draw(ref, 64, 64, 100, 5, threads, [samples], level=6, cell_list=cells, states=st)
    for t in range(threads):
        plain = oracle.Xorwow()
        oracle.lib.orc_xorwow_init(1337, t, 0, C.byref(plain))
        for _ in range(6 * samples):
            oracle.lib.orc_xorwow_next(C.byref(plain))
        assert int(st[t]["d"]) == plain.d and list(st[t]["x"]) == list(plain.x)
