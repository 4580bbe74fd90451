"""make_bin_layout (scatter.hip), swept through cb_debug_scatter_layout on a fake base address: no GPU.

The kernels of the scatter index the workspace's arrays by what the layout says (cap, max_regions, n_groups, ...), and
their grids are upper bounds derived from it; a layout whose arrays overlap, whose rows are misaligned or whose
region table is one too short makes them drop or corrupt entries silently.  Every property below is one a kernel of
scatter.hip or a draw kernel relies on."""

import itertools

import pytest

R = 32768  # entries of a region (one level; chunked: 32 chunks of 1024)
G = R - 8  # entries of a region cut from a group's stretch (two levels, counting sort)
CHUNK = 1024
REGION_CHUNKS = 32
GROUP_TILES = 1024
CHUNKED_GROUPS_MAX = 64
MAX_TILES = 256 * GROUP_TILES
SPT = 50
ENTRIES_PER_SAMPLE = 2.5  # the estimate cb_scatter_workspace_bytes sizes for (x 1.5 for a fused launch of several planes)

# around every threshold of the host code: 256 tiles (few / many), 128 tile columns (lean / general), 1024 tiles (one /
# two levels), 64 groups (chunked / counting sort), 262144 tiles (none), and the 16-bit limits of row and column
CANVASES = [
    (1, 1), (100, 60), (128, 128), (129, 128), (2048, 2048), (2176, 2048), (16384, 128), (16512, 128), (4096, 4096),
    (4224, 4096), (65536, 128), (128, 65536), (16384, 2048), (16384, 2176), (20000, 20000), (65536, 16384),
    (65536, 16512), (65536, 65536),
]
THREADS = [1, 64, 256, 257, 768, 4096, 65536, 262144]
KNOBS = [{}, {"CUDABROT_AMD_TWO_LEVEL": "1"}, {"CUDABROT_AMD_CHUNKED": "0"},
         {"CUDABROT_AMD_TWO_LEVEL": "1", "CUDABROT_AMD_CHUNKED": "0"}]
BASES = [1 << 20, (1 << 20) + 1, (1 << 20) + 255, 0x7F0000000010]
ROW_ALIGNED = ("stream", "sorted", "grouped", "run_start")


def _tiles(w, h, planes):
    return ((w + 127) // 128) * ((h + 127) // 128) * max(planes, 1)


def _worst_regions(layout):
    """The most regions cap * n_waves entries can form.  One level: every wave's segment is cut on its own, ceil(cap /
    R) regions each.  Two levels: every group's stretch is cut on its own into pieces of P (G entries, or 32 chunks),
    and the stretches sum to at most E entries (chunks): sum ceil(T_g / P) is largest when as many groups as can be
    hold 1 modulo P -- n groups of 1 and every further P one more region."""
    if not layout.two_level:
        return layout.n_waves * -(-layout.cap // R)
    if layout.chunked:
        total, piece = layout.n_waves * layout.chunks_per_wave, REGION_CHUNKS
    else:
        total, piece = layout.n_waves * layout.cap, G
    n = min(layout.n_groups, total)
    return n + (total - n) // piece


def _check(cb, layout, base, size, w, h, planes, n_threads, knobs):
    what = (w, h, planes, n_threads, knobs, base, size)
    n_waves = (n_threads + 255) // 256 * 4
    n_tiles = _tiles(w, h, planes)
    assert layout.n_waves == n_waves and layout.n_planes == max(planes, 1), what
    assert layout.n_tiles == n_tiles and layout.tiles_x == (w + 127) // 128 and layout.tiles_y == (h + 127) // 128, what
    # the paths agree with the tile count and the knobs
    two_level = n_tiles > GROUP_TILES or knobs.get("CUDABROT_AMD_TWO_LEVEL") == "1"
    n_groups = -(-n_tiles // GROUP_TILES)
    chunked = two_level and n_groups <= CHUNKED_GROUPS_MAX and knobs.get("CUDABROT_AMD_CHUNKED") != "0"
    assert (layout.two_level, layout.n_groups, layout.chunked) == (int(two_level), n_groups, int(chunked)), what
    # the word has room for every pixel of every plane
    if planes == 0:
        assert (layout.e_row_shift, layout.e_col_mask, layout.e_row_mask, layout.e_chan_mask) == (16, 0xFFFF, 0xFFFF, 0), what
    else:
        assert layout.e_col_mask >= w - 1 and layout.e_row_mask >= h - 1 and layout.e_chan_mask >= planes - 1, what
        assert layout.e_col_mask < 1 << layout.e_row_shift, what
        assert planes == 1 or layout.e_row_mask << layout.e_row_shift < 1 << layout.e_chan_shift, what
        assert layout.e_chan_mask << layout.e_chan_shift < 1 << 32, what
    # segments
    cap = layout.cap
    assert cap % 8 == 0 and cap >= 4096 and cap * n_waves < 1 << 32, what
    if chunked:
        assert cap % CHUNK == 0 and layout.chunks_per_wave * CHUNK == cap, what
    else:
        assert layout.chunks_per_wave == 0, what
    assert layout.max_regions % 8 == 0 and layout.max_regions >= _worst_regions(layout), (what, layout.max_regions)
    # arrays: inside the workspace, disjoint, rows on 16-byte boundaries, large enough for what the kernels index
    arrays = layout.arrays()
    expect = {"wave_count", "stream", "region_start", "region_count", "region_group", "owner_first", "group_first",
              "group_regions", "n_regions", "run_start", "slice_base", "sorted"}
    if two_level:
        expect |= {"a_count", "a_base"}
    if chunked:
        expect |= {"chunk_desc", "chunk_list"}
    elif two_level:
        expect |= {"grouped"}
    assert set(arrays) == expect, what
    spans = sorted((off, off + n, name) for name, (off, n) in arrays.items())
    assert spans[0][0] >= 0 and spans[-1][1] <= size, (what, spans)
    for (_, end, a), (begin, _, b) in zip(spans, spans[1:]):
        assert end <= begin, (what, a, b)
    for name in ROW_ALIGNED:
        if name in arrays:
            assert (base + arrays[name][0]) % 16 == 0, (what, name)
    assert (base + arrays["chunk_list"][0]) % 8 == 0 if chunked else True, what
    assert (base + arrays["region_start"][0]) % 8 == 0 and (base + arrays["a_base"][0]) % 8 == 0 if two_level else True, what
    rows = min(n_tiles, GROUP_TILES)
    keys = n_groups if chunked else n_groups * 4
    need = {
        "wave_count": 4 * n_waves, "stream": 4 * cap * n_waves, "region_start": 8 * layout.max_regions,
        "region_count": 4 * layout.max_regions, "region_group": 4 * layout.max_regions,
        "owner_first": 4 * (max(n_waves, n_groups) + 1), "group_first": 4 * n_groups, "group_regions": 4 * n_groups,
        "n_regions": 16, "run_start": 2 * rows * layout.max_regions, "slice_base": 4 * (n_tiles + 1),
        "sorted": 2 * (layout.max_regions * R if chunked else cap * n_waves),
    }
    if two_level:
        need.update(a_count=4 * keys * n_waves, a_base=8 * (keys + 1))
    if chunked:
        need.update(chunk_desc=4 * n_waves * layout.chunks_per_wave, chunk_list=8 * n_waves * layout.chunks_per_wave)
    elif two_level:
        need.update(grouped=4 * cap * n_waves)
    for name, n in need.items():
        assert arrays[name][1] >= n, (what, name, arrays[name], n)
    # the region sort's 16-byte loads may read up to three words past a segment or a stretch: still inside
    for name in ("stream", "grouped"):
        if name in arrays:
            assert arrays[name][0] + arrays[name][1] + 12 <= size, (what, name)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "+".join(sorted(k)) or "default")
@pytest.mark.parametrize("planes", [0, 1, 2, 3, 4])
def test_every_layout_of_the_sweep_is_sound(cb, monkeypatch, planes, knobs):
    for name in ("CUDABROT_AMD_TWO_LEVEL", "CUDABROT_AMD_CHUNKED", "CUDABROT_AMD_SLICE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    enabled = 0
    for (w, h), n_threads in itertools.product(CANVASES, THREADS):
        dims = cb.FractalDimensions.make(w, h)
        suggested = cb.scatter_workspace_bytes(dims, n_threads, SPT, n_channels=max(planes, 1))
        word_bits = (w - 1).bit_length() + (h - 1).bit_length() + (planes - 1).bit_length() if planes else 32
        can = _tiles(w, h, planes) <= MAX_TILES and word_bits <= 32
        if _tiles(w, h, planes) > MAX_TILES:
            assert suggested == 0, (w, h, planes)
        sizes = [0, 4096] + ([suggested, suggested // 3, suggested - 1, suggested + 1, suggested - 255, suggested + 255]
                             if suggested else [1 << 30])
        for k, size in enumerate(sizes):
            for base in (BASES if k == 2 else BASES[k % 2::2]):
                layout = cb.debug_scatter_layout(dims, n_threads, base, size, n_channels=planes)
                what = (w, h, planes, n_threads, knobs, base, size)
                if not can or size <= 4096:
                    assert not layout.enabled and not layout.arrays() and layout.cap == 0, what
                    continue
                if size >= suggested - 255 and base % 256 == 0:
                    # (a base off the 256-byte grid costs up to 255 bytes of the workspace)
                    assert layout.enabled, what
                    if size >= suggested:
                        sized_for = n_threads * SPT * ENTRIES_PER_SAMPLE * (1.5 if planes > 1 else 1.0)
                        assert layout.cap * layout.n_waves >= sized_for, (what, layout.cap)
                if layout.enabled:
                    enabled += 1
                    _check(cb, layout, base, size, w, h, planes, n_threads, knobs)
                else:
                    assert not layout.arrays() and layout.cap == 0, what
    assert enabled > 500


def test_the_query_rejects_bad_arguments_and_ignores_the_workspace(cb):
    import ctypes as C

    dims = cb.FractalDimensions.make(640, 480)
    out = cb.ScatterLayout()
    bad = 1  # hipErrorInvalidValue
    assert cb.lib.cb_debug_scatter_layout(None, 0, 256, 4096, 1 << 24, C.byref(out)) == bad
    assert cb.lib.cb_debug_scatter_layout(C.byref(dims), 0, 256, 4096, 1 << 24, None) == bad
    assert cb.lib.cb_debug_scatter_layout(C.byref(dims), -1, 256, 4096, 1 << 24, C.byref(out)) == bad
    assert cb.lib.cb_debug_scatter_layout(C.byref(dims), 5, 256, 4096, 1 << 24, C.byref(out)) == bad
    empty = cb.FractalDimensions(0, 480, -2.0, -2.0, 2.0, 2.0, 0.0, 0.0)
    assert cb.lib.cb_debug_scatter_layout(C.byref(empty), 0, 256, 4096, 1 << 24, C.byref(out)) == bad
    # no workspace, no threads: a layout that is not enabled, not an error
    assert not cb.debug_scatter_layout(dims, 256, 0, 1 << 24).enabled
    assert not cb.debug_scatter_layout(dims, 0, 4096, 1 << 24).enabled
    # the same answer wherever the (256-byte aligned) workspace lies: offsets, not addresses
    a = cb.debug_scatter_layout(dims, 768, 1 << 12, 1 << 24)
    b = cb.debug_scatter_layout(dims, 768, 1 << 40, 1 << 24)
    assert a.enabled and bytes(a) == bytes(b)
    # a four-plane word of 16 + 16 + 2 bits has no room: direct atomics, whatever the workspace
    huge = cb.FractalDimensions.make(65536, 65536)
    assert not cb.debug_scatter_layout(huge, 768, 1 << 12, 1 << 40, n_channels=4).enabled
