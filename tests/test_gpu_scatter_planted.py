"""The tile-binned scatter (scatter.hip) on streams planted for it, against a bincount (tests/scatter_reference.py).

Everywhere else in the suite the scatter sorts what a draw kernel wrote: Mandelbrot orbits, which decide the edges
that get hit.  cb_flush_scatter[_channels] is stateless -- it rebuilds the layout from its arguments and sorts what
the workspace holds -- so here the test writes wave_count, chunk_desc and the stream itself, where
cb_debug_scatter_layout says they lie, and chooses the edges: wave segments of exactly a region and one more, group
stretches that make the next region start on every residue of a 16-byte boundary, regions of exactly 32 and 33 chunks,
a tile that receives a whole region, row and column 65535, a group that ends inside a colour plane, a stream of
nothing.  One flush per case; the histogram, prefilled with distinct large counts, must equal the reference bit for
bit.  Only streams inside the producer contract: what the draw kernels never write pins nothing.

The workspace is filled with scatter_reference.STALE_BYTE first: whatever lies beyond the planted words is stale, is
not zero, and must not be counted.
"""

import functools

import numpy as np
import pytest

import scatter_reference as ref

pytestmark = pytest.mark.gpu

R = 32768            # entries of a region of a wave's segment
G = R - 8            # entries of a region of a group's stretch (two levels, counting sort)
C = ref.CHUNK_WORDS  # words of a chunk
N_WAVES = 12         # the fills below cycle over the waves (12 is a multiple of the draw kernel's 4 per workgroup)
CAP_TARGET = 3 * R + R // 2 + 8  # a segment of three regions and a partial one
DEVICE = "cuda:0"
KNOBS = ("CUDABROT_AMD_TWO_LEVEL", "CUDABROT_AMD_CHUNKED", "CUDABROT_AMD_SLICE")
PATTERNS = ["uniform", "pixel", "tile", "ends", "edges", "sorted"]


# ---- pixels ---------------------------------------------------------------------------------------------------------

def _in_tiles(L, w, h, tiles, rng):
    """A random pixel inside each of `tiles` (indices into the stack of planes) -> (plane, row, col)."""
    tiles = np.asarray(tiles, dtype=np.int64)
    per_plane = L.tiles_x * L.tiles_y
    plane, rem = tiles // per_plane, tiles % per_plane
    r0, c0 = (rem // L.tiles_x) * 128, (rem % L.tiles_x) * 128
    rows, cols = np.minimum(128, h - r0), np.minimum(128, w - c0)
    row = r0 + rng.integers(0, 1 << 30, tiles.size) % rows
    col = c0 + rng.integers(0, 1 << 30, tiles.size) % cols
    return plane, row, col


def _last_pixel(L, w, h, tile):
    plane, row, col = _in_tiles(L, w, h, [tile], np.random.default_rng(0))
    return plane, np.minimum(row // 128 * 128 + 127, h - 1), np.minimum(col // 128 * 128 + 127, w - 1)


def _pixels(pattern, n, L, w, h, rng, lo=0, hi=None):
    """n pixels of a pattern inside the tiles [lo, hi) (default: the whole stack of planes) -> (plane, row, col)."""
    whole = hi is None
    hi = L.n_tiles if whole else hi
    if n == 0:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    if pattern == "uniform":  # over the canvas (over the tiles of a group)
        if whole:
            return rng.integers(0, L.n_planes, n), rng.integers(0, h, n), rng.integers(0, w, n)
        return _in_tiles(L, w, h, rng.integers(lo, hi, n), rng)
    if pattern == "pixel":    # the last pixel of all: (h - 1, w - 1) of the last plane
        return tuple(np.repeat(v, n) for v in _last_pixel(L, w, h, hi - 1))
    if pattern == "tile":     # one tile receives everything
        return _in_tiles(L, w, h, np.full(n, lo + 2 * (hi - 1 - lo) // 3), rng)
    if pattern == "ends":     # alternately the first and the last tile
        return _in_tiles(L, w, h, np.where(np.arange(n) % 2 == 0, lo, hi - 1), rng)
    if pattern == "edges":    # rows and columns beside a tile boundary and the canvas' edge only
        rows = sorted({v for v in (0, 127, 128, h - 1) if v < h})
        cols = sorted({v for v in (0, 127, 128, w - 1) if v < w})
        grid = np.array([(p, r, c) for p in range(L.n_planes) for r in rows for c in cols], dtype=np.int64)
        tile = ref.tile_of(L, grid[:, 0], grid[:, 1], grid[:, 2])
        grid = grid[(tile >= lo) & (tile < hi)]
        if not len(grid):     # a group of tile rows without such a pixel
            return _pixels("uniform", n, L, w, h, rng, lo, hi)
        pick = grid[rng.integers(0, len(grid), n)]
        return pick[:, 0], pick[:, 1], pick[:, 2]
    if pattern == "sorted":   # tile by tile, tile % 17 + 1 entries each: run boundaries on every residue modulo 8
        tiles = np.arange(lo, hi)
        once = np.repeat(tiles, tiles % 17 + 1)
        return _in_tiles(L, w, h, np.resize(once, n), rng)
    raise ValueError(pattern)


def _concat(parts):
    parts = list(parts)
    return tuple(np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=np.int64) for k in range(3))


def _group_tiles(L, g):
    return g * 1024, min((g + 1) * 1024, L.n_tiles)


# ---- one case -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _start(n):
    start = ref.prefill(n)
    start.setflags(write=False)
    return start


class Case:
    """A workspace whose segments hold between 3 and 5 regions, and its layout."""

    def __init__(self, cb, monkeypatch, w, h, planes=0, knobs=None, n_waves=N_WAVES):
        import torch

        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        for name, value in (knobs or {}).items():
            monkeypatch.setenv(name, value)
        self.cb, self.w, self.h, self.planes = cb, w, h, planes
        self.dims = cb.FractalDimensions.make(w, h)
        self.n_threads = n_waves * 64
        lo, hi = 0, 1 << 34  # the smallest workspace whose cap reaches the target (cap is read, never computed)
        while hi - lo > 256:
            mid = (lo + hi) // 2
            at = cb.debug_scatter_layout(self.dims, self.n_threads, 1 << 20, mid, n_channels=planes)
            lo, hi = (lo, mid) if at.enabled and at.cap >= CAP_TARGET else (mid, hi)
        self.bytes = hi
        self.ws = torch.full((self.bytes,), ref.STALE_BYTE, dtype=torch.uint8, device=DEVICE)
        self.L = L = cb.debug_scatter_layout(self.dims, self.n_threads, self.ws.data_ptr(), self.bytes, n_channels=planes)
        assert L.enabled and L.n_waves == n_waves and 3 * R <= L.cap <= 5 * R, (L.enabled, L.n_waves, L.cap)

    def _write(self, name, values):
        import torch

        off, n = self.L.arrays()[name]
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        assert raw.size == n and 0 <= off and off + n <= self.bytes, (name, raw.size, off, n)
        self.ws[off: off + n] = torch.from_numpy(raw).to(self.ws.device)

    def flush_and_check(self, pixels_per_wave, note=""):
        """Plants the waves' pixels, flushes once, and requires start + bincount."""
        import torch

        cb, L, w, h = self.cb, self.L, self.w, self.h
        if L.chunked:
            counts, desc, stream = ref.place_chunked(L, pixels_per_wave)
            self._write("chunk_desc", desc)
        else:
            counts, stream = ref.place_plain(L, [ref.pack_words(L, *p) for p in pixels_per_wave])
        self._write("wave_count", counts)
        self._write("stream", stream)
        start = _start(L.n_planes * w * h)
        expected = ref.expected_histogram(start, w, h, *_concat(pixels_per_wave))
        hist = torch.arange(start.size, dtype=torch.int64, device=self.ws.device) * 3 + (1 << 40)
        if self.planes:
            cb.flush_scatter_channels(self.dims, hist.data_ptr(), self.planes, self.n_threads, self.ws.data_ptr(), self.bytes)
        else:
            cb.flush_scatter(self.dims, hist.data_ptr(), self.n_threads, self.ws.data_ptr(), self.bytes)
        torch.cuda.synchronize(hist.device)
        want = torch.from_numpy(expected.view(np.int64)).to(hist.device)
        if not torch.equal(hist, want):
            bad = torch.nonzero(hist != want).reshape(-1)
            first = [(int(i) // (w * h), int(i) % (w * h) // w, int(i) % w, int(hist[i] - want[i])) for i in bad[:8]]
            pytest.fail("%d entries planted, %d pixels differ; first (plane, row, col, got - expected): %s; counts per "
                        "wave %s; cap %d%s" % (sum(len(p[0]) for p in pixels_per_wave), bad.numel(), first,
                                               counts.tolist(), L.cap, note))


# ---- the fills ------------------------------------------------------------------------------------------------------

def _wave_fills(cap):
    return [0, 1, 7, 8, 9, R - 1, R, R + 1, 2 * R, 2 * R + 5, cap]


def _plain_waves(case, pattern, rng, fills=None):
    L = case.L
    fills = fills or _wave_fills(L.cap)
    return [_pixels(pattern, fills[k % len(fills)], L, case.w, case.h, rng) for k in range(L.n_waves)]


def _deal(pixels, L, rng):
    """All words of a launch, shuffled and cut into the waves' segments at random places (none beyond cap)."""
    n = len(pixels[0])
    order = rng.permutation(n)
    cuts = np.sort(rng.integers(0, n + 1, L.n_waves - 1))
    if n and np.diff(np.concatenate([[0], cuts, [n]])).max() > L.cap:
        cuts = np.arange(1, L.n_waves) * n // L.n_waves
    assert n <= L.n_waves * L.cap and (not n or np.diff(np.concatenate([[0], cuts, [n]])).max() <= L.cap)
    return [tuple(v[part] for v in pixels) for part in np.split(order, cuts)]


def _grouped_waves(case, pattern, totals, rng):
    """Two levels, counting sort: totals[g] words of group g in all, mixed over the waves."""
    L = case.L
    assert len(totals) == L.n_groups
    return _deal(_concat(_pixels(pattern, n, L, case.w, case.h, rng, *_group_tiles(L, g)) for g, n in enumerate(totals)),
                 L, rng)


def _chunk_waves(case, pattern, words, rng):
    """Chunked: words[w][g] words of group g in wave w (place_chunked cuts them into chunks)."""
    L = case.L
    return [_concat(_pixels(pattern, int(n), L, case.w, case.h, rng, *_group_tiles(L, g)) for g, n in enumerate(row))
            for row in words]


def _chunks_per_wave_plan(L):
    """Waves in turn: no chunk, one chunk of 1, of 1023, of 1024 words, every chunk of the segment opened."""
    words = np.zeros((L.n_waves, L.n_groups), dtype=np.int64)
    for w in range(L.n_waves):
        kind, g = w % 5, w % L.n_groups
        if kind in (1, 2, 3):
            words[w][g] = (1, C - 1, C)[kind - 1]
        elif kind == 4:
            share = [L.chunks_per_wave // L.n_groups + (k < L.chunks_per_wave % L.n_groups) for k in range(L.n_groups)]
            for k, chunks in enumerate(share):  # the last chunk of every group partial, of the last group full
                words[w][k] = (chunks - 1) * C + (C if k == L.n_groups - 1 else 1 + 341 * (w + k) % C)
    return words


def _chunk_totals_plan(L, totals):
    """totals[g] chunks of group g over all waves, as evenly as they go; last chunks of 1, 1023, 1024, ... words."""
    words = np.zeros((L.n_waves, L.n_groups), dtype=np.int64)
    for g, total in enumerate(totals):
        for w in range(L.n_waves):
            chunks = total // L.n_waves + (w < total % L.n_waves)
            if chunks:
                words[w][g] = (chunks - 1) * C + (1, C - 1, C, 512)[(w + g) % 4]
    assert (np.ceil(words / C).sum(axis=1) <= L.chunks_per_wave).all()
    return words


def _fill_for_path(case, pattern, rng, variant=0):
    """The waves of a case on whatever path the canvas takes (fused canvases: the path is the layout's)."""
    L = case.L
    if L.chunked:
        return _chunk_waves(case, pattern, _chunks_per_wave_plan(L), rng)
    if L.two_level:
        return _grouped_waves(case, pattern, _group_totals(L.n_groups)[variant], rng)
    return _plain_waves(case, pattern, rng)


# ---- one level, plain -----------------------------------------------------------------------------------------------

ONE_LEVEL = [
    (100, 60), (128, 128), (2048, 2048), (128, 65536),    # lean, few tiles (the last: row 65535)
    (2176, 2048), (16384, 128), (4096, 4096),            # lean, many tiles (272; 128 tile columns; 1024 tiles)
    (16512, 128), (65536, 128),                          # general: more than 128 tile columns, column 65535
]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("canvas", ONE_LEVEL, ids=lambda c: "%dx%d" % c)
def test_one_level_plain(cb, monkeypatch, canvas, pattern):
    case = Case(cb, monkeypatch, *canvas)
    assert not case.L.two_level and case.L.n_planes == 1
    case.flush_and_check(_plain_waves(case, pattern, np.random.default_rng(1)))


# ---- two levels, counting sort --------------------------------------------------------------------------------------

def _group_totals(n_groups):
    """Per-group totals over all waves.  One group: each edge.  Two: the first group's total on residues 1, 4 and 7
    modulo 8 (the second group's stretch, and every region cut from it, then starts off a 16-byte boundary), then on
    0 and 3 and empty, beside every edge of the second."""
    if n_groups == 1:
        return [(1,), (G - 1,), (G,), (G + 1,), (2 * G + 3,)]
    assert n_groups == 2
    return [(1, 2 * G + 3), (G + 4, G), (G - 1, G + 1), (2 * G + 3, G - 1), (G, 1), (0, 2 * G + 3), (G + 1, 0),
            (2 * G + 7, G + 1), (5, G)]


COUNTING = [(2176, 2048, {"CUDABROT_AMD_TWO_LEVEL": "1", "CUDABROT_AMD_CHUNKED": "0"}, 1),  # one partial group
            (4224, 4096, {"CUDABROT_AMD_CHUNKED": "0"}, 2)]                                 # 1024 + 32 tiles


def _counting_cases():
    """Every pattern meets every residue of the first group (the first three totals of two groups); the other totals
    take the patterns in turn.  One group: every pattern, every total."""
    for canvas in COUNTING:
        for variant in range(len(_group_totals(canvas[3]))):
            for k, pattern in enumerate(PATTERNS):
                if canvas[3] == 1 or variant < 3 or (variant - 3) % len(PATTERNS) == k:
                    yield pytest.param(canvas, pattern, variant, id="%dx%d-%s-%d" % (canvas[0], canvas[1], pattern, variant))


@pytest.mark.parametrize("canvas,pattern,variant", _counting_cases())
def test_two_levels_counting_sort(cb, monkeypatch, canvas, pattern, variant):
    w, h, knobs, n_groups = canvas
    totals = _group_totals(n_groups)[variant]
    case = Case(cb, monkeypatch, w, h, knobs=knobs)
    assert case.L.two_level and not case.L.chunked and case.L.n_groups == n_groups
    case.flush_and_check(_grouped_waves(case, pattern, totals, np.random.default_rng(2)), " totals %s" % (totals,))


# ---- two levels, chunked --------------------------------------------------------------------------------------------

CHUNKED = [(700, 500, {"CUDABROT_AMD_TWO_LEVEL": "1"}), (4224, 4096, {}), (16384, 2048, {}), (16384, 2176, {})]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("canvas", CHUNKED, ids=lambda c: "%dx%d" % c[:2])
def test_chunked_chunks_per_wave(cb, monkeypatch, canvas, pattern):
    w, h, knobs = canvas
    case = Case(cb, monkeypatch, w, h, knobs=knobs)
    assert case.L.chunked
    case.flush_and_check(_chunk_waves(case, pattern, _chunks_per_wave_plan(case.L), np.random.default_rng(3)))


@pytest.mark.parametrize("turn", range(4))
@pytest.mark.parametrize("canvas", CHUNKED, ids=lambda c: "%dx%d" % c[:2])
def test_chunked_chunks_per_group(cb, monkeypatch, canvas, turn):
    """31, 32, 33 and 65 chunks of a group in all: a region of 32 chunks less one, exactly one, one and a chunk, two
    and a chunk.  Every total meets every group of every canvas."""
    w, h, knobs = canvas
    case = Case(cb, monkeypatch, w, h, knobs=knobs)
    totals = [(31, 32, 33, 65)[(g + turn) % 4] for g in range(case.L.n_groups)]
    pattern = PATTERNS[(turn + len(CHUNKED) * CHUNKED.index(canvas)) % len(PATTERNS)]
    case.flush_and_check(_chunk_waves(case, pattern, _chunk_totals_plan(case.L, totals), np.random.default_rng(4)),
                         " chunks per group %s, %s" % (totals, pattern))


# ---- fused planes ---------------------------------------------------------------------------------------------------

FUSED = [
    (1, 200, 100, {}),            # a word that is not the plain one: narrow fields
    (3, 200, 100, {}),
    (4, 2048, 2048, {}),          # 1024 tiles: the most of one level
    (4, 2176, 2048, {}),          # 1088 tiles, chunked: group 0 ends inside plane 3
    (4, 2176, 2048, {"CUDABROT_AMD_CHUNKED": "0"}),
]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("canvas", FUSED, ids=lambda c: "%dx%dx%d%s" % (c[0], c[1], c[2], "-counting" if c[3] else ""))
def test_fused_planes(cb, monkeypatch, canvas, pattern):
    planes, w, h, knobs = canvas
    case = Case(cb, monkeypatch, w, h, planes=planes, knobs=knobs)
    L = case.L
    assert L.n_planes == planes and (L.e_row_shift, L.e_col_mask) != (16, 0xFFFF)
    assert (L.two_level, L.chunked) == (int(w == 2176), int(w == 2176 and not knobs))
    case.flush_and_check(_fill_for_path(case, pattern, np.random.default_rng(5), variant=PATTERNS.index(pattern)))


def test_four_planes_of_65536_squared_have_no_layout(cb, monkeypatch):
    """16 + 16 + 2 bits do not fit a word: the query says so for a workspace of any size (none is allocated), the draw
    kernel then adds with direct atomics and the flush has nothing to do."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    dims = cb.FractalDimensions.make(65536, 65536)
    for size in (1 << 20, 1 << 32, 1 << 40):
        L = cb.debug_scatter_layout(dims, N_WAVES * 64, 1 << 20, size, n_channels=4)
        assert not L.enabled and not L.arrays()


# ---- nothing, slices, random ----------------------------------------------------------------------------------------

PATHS = {
    "lean-few": (2048, 2048, 0, {}),
    "lean-many": (4096, 4096, 0, {}),
    "general": (65536, 128, 0, {}),
    "counting": (4224, 4096, 0, {"CUDABROT_AMD_CHUNKED": "0"}),
    "chunked": (16384, 2176, 0, {}),
    "fused": (3, 200, 100, {}),
    "fused-chunked": (4, 2176, 2048, {}),
}


def _path_case(cb, monkeypatch, path, n_waves=N_WAVES):
    a, b, c, knobs = PATHS[path]
    w, h, planes = (b, c, a) if path.startswith("fused") else (a, b, c)
    return Case(cb, monkeypatch, w, h, planes=planes, knobs=knobs, n_waves=n_waves)


@pytest.mark.parametrize("path", PATHS)
def test_an_empty_stream_leaves_the_histogram_alone(cb, monkeypatch, path):
    case = _path_case(cb, monkeypatch, path)
    none = tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    case.flush_and_check([none] * case.L.n_waves)


@pytest.mark.parametrize("slice_regions", [None, "1", "3"])
def test_slices_of_a_tile(cb, monkeypatch, slice_regions):
    """46 regions (eleven full segments and one of a region and an entry) on 1024 tiles, gathered one region, three
    regions (a partial last slice) and 512 at a time: with one region per workgroup the gather's grid is at its bound."""
    case = Case(cb, monkeypatch, 4096, 4096, knobs={"CUDABROT_AMD_SLICE": slice_regions} if slice_regions else None)
    L = case.L
    regions = -(-L.cap // R)
    assert (L.n_waves - 1) * regions + 2 >= 40
    waves = _plain_waves(case, "uniform", np.random.default_rng(6), fills=[L.cap] * (L.n_waves - 1) + [R + 1])
    case.flush_and_check(waves, " slice %s" % slice_regions)


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("path", PATHS)
def test_random_streams(cb, monkeypatch, path, seed):
    rng = np.random.default_rng(seed)
    case = _path_case(cb, monkeypatch, path, n_waves=int(rng.choice([12, 16, 20])))
    L = case.L
    if L.chunked:  # per wave: a random number of chunks, dealt to random groups; every group's last chunk partial
        words = np.zeros((L.n_waves, L.n_groups), dtype=np.int64)
        for w in range(L.n_waves):
            chunks = rng.multinomial(rng.integers(0, L.chunks_per_wave + 1) if rng.random() < 0.8 else 0,
                                     np.ones(L.n_groups) / L.n_groups)
            words[w] = [(c - 1) * C + rng.integers(1, C + 1) if c else 0 for c in chunks]
        waves = _chunk_waves(case, "uniform", words, rng)
    else:
        fills = [int(rng.integers(0, L.cap + 1)) if rng.random() < 0.8 else 0 for _ in range(L.n_waves)]
        waves = _plain_waves(case, "uniform", rng, fills=fills)
    case.flush_and_check(waves, " seed %d" % seed)
