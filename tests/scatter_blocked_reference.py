"""The BLOCKED form of a one-level pixel stream (cudabrot_amd/csrc/kernels.h, kStreamBlocked), restated for tests that
plant one.  Beside tests/scatter_reference.py, which states the plain and the chunked forms and stays as it is.

  blocked segment  wave_count[w] = slots | 1 << 31, slots a multiple of 4 and <= cap; the slots lie at
                   stream[w * cap ...] in blocks of four (16 bytes on a 16-byte boundary: cap is a multiple of 8); a slot
                   holds a word row << 16 | col or the sentinel 0xFFFFFFFF, which names no pixel
  plain segment    wave_count[w] = words, bit 31 clear (scatter_reference.place_plain's)

A workspace may mix the two, segment by segment.  The draw kernel only writes blocks that hold a point; the scatter takes
any block, one of four sentinels included.  The contract is the plain one's: every word that is not the sentinel adds one
to the pixel it names -- the reference is a bincount over them.
"""

import numpy as np

import scatter_reference as ref

BLOCKED = 1 << 31
SENTINEL = 0xFFFFFFFF
BLOCK = 4


def blocks_of(words, masks):
    """The slots of len(masks) blocks: block b holds, in the slots whose bit is set in masks[b] (bit j: slot j), the next
    words of `words` in order, and the sentinel in the others.  -> u32[4 * len(masks)].  `words` must hold exactly as
    many words as the masks have bits."""
    masks = np.asarray(masks, dtype=np.int64)
    real = ((masks[:, None] >> np.arange(BLOCK)) & 1).astype(bool).reshape(-1)
    words = np.asarray(words, dtype=np.uint32)
    assert int(real.sum()) == words.size, (int(real.sum()), words.size)
    slots = np.full(real.size, SENTINEL, dtype=np.uint32)
    slots[real] = words
    return slots


def place_segments(layout, segments):
    """segments[w] = (blocked, u32 slots or words) -> (wave_count u32[n_waves], stream u32[n_waves * cap]); what the
    segments do not cover is scatter_reference.STALE_WORD."""
    assert not layout.chunked and not layout.two_level and len(segments) == layout.n_waves
    assert layout.cap % 8 == 0 and layout.cap < BLOCKED
    counts = np.zeros(layout.n_waves, dtype=np.uint32)
    stream = np.full(layout.n_waves * layout.cap, ref.STALE_WORD, dtype=np.uint32)
    for w, (blocked, slots) in enumerate(segments):
        slots = np.asarray(slots, dtype=np.uint32)
        assert slots.size <= layout.cap and (not blocked or slots.size % BLOCK == 0)
        assert blocked or not (slots == SENTINEL).any()  # (no one-level canvas has row and column 65535)
        counts[w] = slots.size | (BLOCKED if blocked else 0)
        stream[w * layout.cap: w * layout.cap + slots.size] = slots
    return counts, stream


def pixels_of(segments):
    """(row, col) of every word of the segments that names a pixel."""
    words = np.concatenate([np.asarray(s, dtype=np.uint32) for _, s in segments] or [np.zeros(0, np.uint32)])
    words = words[words != SENTINEL].astype(np.int64)
    return words >> 16, words & 0xFFFF
