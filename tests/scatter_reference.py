"""The plain reference of the tile-binned scatter (cudabrot_amd/csrc/scatter.hip), for tests that plant a stream.

The scatter's contract is: every word of the stream adds one to the pixel it names.  The reference is therefore a
bincount over the pixels, and knows nothing of regions, groups, runs or slices.  What it shares with the product is
the FORMAT of the input, which it takes from cb_debug_scatter_layout (a cudabrot_amd.ScatterLayout, `layout` below)
and from the producer contract of DESIGN.md 7 ("Diagnostics and test knobs"):

  plain stream    wave_count[w] <= cap words at stream[w * cap ...]
  chunked stream  wave_count[w] <= chunks_per_wave opened chunks; chunk j of wave w is the 1024 words at
                  stream[w * cap + j * 1024 ...] and chunk_desc[w][j] = group << 16 | words, 1 <= words <= 1024;
                  every word of a chunk belongs to the chunk's group; of the chunks of one (wave, group) only the
                  last one opened is partial

The group of a word is tile >> 10 with tile = (plane * tiles_y + row // 128) * tiles_x + col // 128: the one piece of
the product's arithmetic restated here, because the chunked contract is stated in it.
"""

import numpy as np

TILE = 128
GROUP_SHIFT = 10
CHUNK_WORDS = 1024
# What the helpers leave in every word they do not plant: the scatter must ignore it.  Both 16-bit halves are valid
# in-tile offsets (0x2a2a < 128 * 128), so that a stale word a broken kernel did count still lands inside its tile.
STALE_BYTE = 0x2A
STALE_WORD = 0x2A2A2A2A


def prefill(n):
    """The starting histogram: distinct, large, non-zero counts -- a store in place of an add, or an add to the wrong
    pixel, changes the result."""
    return (np.uint64(1) << np.uint64(40)) + np.uint64(3) * np.arange(n, dtype=np.uint64)


def pack_words(layout, plane, row, col):
    """(plane, row, col) -> stream words of this layout's format."""
    plane, row, col = (np.asarray(v, dtype=np.uint64) for v in (plane, row, col))
    if plane.size:
        assert int(col.max()) <= layout.e_col_mask and int(row.max()) <= layout.e_row_mask
        assert int(plane.max()) <= layout.e_chan_mask
    word = (plane << np.uint64(layout.e_chan_shift)) | (row << np.uint64(layout.e_row_shift)) | col
    assert not word.size or int(word.max()) < 1 << 32
    return word.astype(np.uint32)


def expected_histogram(start, w, h, plane, row, col):
    """start (u64, planes * h * w) + one per (plane, row, col)."""
    index = (np.asarray(plane, dtype=np.int64) * h + np.asarray(row, dtype=np.int64)) * w + np.asarray(col, dtype=np.int64)
    assert not index.size or (int(index.min()) >= 0 and int(index.max()) < start.size)
    return start + np.bincount(index, minlength=start.size).astype(np.uint64)


def tile_of(layout, plane, row, col):
    plane, row, col = (np.asarray(v, dtype=np.int64) for v in (plane, row, col))
    return (plane * layout.tiles_y + row // TILE) * layout.tiles_x + col // TILE


def place_plain(layout, words_per_wave):
    """A plain stream: (wave_count u32[n_waves], stream u32[n_waves * cap]) holding words_per_wave[w] as wave w's."""
    assert not layout.chunked and len(words_per_wave) == layout.n_waves
    counts = np.zeros(layout.n_waves, dtype=np.uint32)
    stream = np.full(layout.n_waves * layout.cap, STALE_WORD, dtype=np.uint32)
    for w, words in enumerate(words_per_wave):
        assert len(words) <= layout.cap
        counts[w] = len(words)
        stream[w * layout.cap: w * layout.cap + len(words)] = words
    return counts, stream


def place_chunked(layout, pixels_per_wave):
    """A chunked stream: (wave_count, chunk_desc u32[n_waves * chunks_per_wave], stream).  pixels_per_wave[w] is wave
    w's (plane, row, col); its words are split by group into chunks (full ones, then the group's partial one), and
    the groups' chunks are dealt into the wave's descriptor row in turn, so that the groups interleave there."""
    assert layout.chunked and len(pixels_per_wave) == layout.n_waves
    cpw = layout.chunks_per_wave
    counts = np.zeros(layout.n_waves, dtype=np.uint32)
    desc = np.full(layout.n_waves * cpw, STALE_WORD, dtype=np.uint32)
    stream = np.full(layout.n_waves * layout.cap, STALE_WORD, dtype=np.uint32)
    for w, (plane, row, col) in enumerate(pixels_per_wave):
        words = pack_words(layout, plane, row, col)
        group = tile_of(layout, plane, row, col) >> GROUP_SHIFT
        chunks = {}  # group -> its chunks, in the order they are opened
        for g in np.unique(group):
            mine = words[group == g]
            chunks[int(g)] = [mine[i: i + CHUNK_WORDS] for i in range(0, len(mine), CHUNK_WORDS)]
        row_of_chunks = []
        while any(chunks.values()):
            for g in sorted(chunks):
                if chunks[g]:
                    row_of_chunks.append((g, chunks[g].pop(0)))
        assert len(row_of_chunks) <= cpw, (len(row_of_chunks), cpw)
        counts[w] = len(row_of_chunks)
        for j, (g, chunk) in enumerate(row_of_chunks):
            assert 1 <= len(chunk) <= CHUNK_WORDS and g < layout.n_groups
            desc[w * cpw + j] = (g << 16) | len(chunk)
            at = w * layout.cap + j * CHUNK_WORDS
            stream[at: at + len(chunk)] = chunk
    return counts, desc, stream
