"""The tile-binned scatter (scatter.hip) on BLOCKED streams planted for it (kernels.h, kStreamBlocked: what
draw_wide_kernel writes on a one-level canvas), against a bincount (tests/scatter_blocked_reference.py).

Driven as tests/test_gpu_scatter_planted.py drives the plain streams -- its Case, its pixel patterns, one flush per case,
a prefilled histogram that must come out bit for bit -- with segments that say, by bit 31 of their wave_count, that they
are rows of blocks of four slots, some of which hold the sentinel.  The shapes are the ones the draw kernel does not
choose often or at all: the sentinel at every position of a block, blocks of which only the last slot is real, regions
(a full one and a partial one) that END in blocks of nothing but sentinels -- where the last tile's run must end at the
entries placed, not at the slots read --, segments of exactly one region and of a region and a block, an empty blocked
segment, and plain segments beside them in the same workspace.
"""

import numpy as np
import pytest

import scatter_blocked_reference as blk
import scatter_reference as ref
from test_gpu_scatter_planted import Case, R, _pixels, _start

pytestmark = pytest.mark.gpu

CANVASES = [(256, 256), (1000, 1000), (4096, 4096)]  # 4 tiles; 64 tiles (the eight-replica counters); 1024 tiles
PATTERNS = ["uniform", "pixel", "sorted"]            # "pixel": everything in the LAST tile, whose run ends the image


def _words(case, pattern, n, rng):
    plane, row, col = _pixels(pattern, n, case.L, case.w, case.h, rng)
    return ref.pack_words(case.L, plane, row, col)


def _blocked(case, pattern, masks, rng):
    masks = np.asarray(masks, dtype=np.int64)
    bits = int(((masks[:, None] >> np.arange(blk.BLOCK)) & 1).sum())  # the points the blocks hold
    return True, blk.blocks_of(_words(case, pattern, bits, rng), masks)


def _plain(case, pattern, n, rng):
    return False, _words(case, pattern, n, rng)


def _segments(case, pattern, rng):
    """Twelve segments (Case's N_WAVES), every shape of the module's text among them."""
    cap = case.L.cap
    every = np.arange(R // 2) % 15 + 1                      # masks 1 .. 15 in turn: a sentinel at every position
    random = lambda blocks: rng.integers(1, 16, blocks)     # noqa: E731  (no block of four sentinels)
    tail = lambda blocks, empty: np.concatenate([random(blocks - empty), np.zeros(empty, dtype=np.int64)])  # noqa: E731
    return [
        _blocked(case, pattern, every, rng),                # two regions
        _blocked(case, pattern, np.full(R // 4, 8), rng),   # exactly one region; only the last slot of a block is real
        _blocked(case, pattern, random(R // 4 + 1), rng),   # a region and one block
        _blocked(case, pattern, tail(R // 4 + R // 8, 1000), rng),  # the last, PARTIAL region ends in 1000 empty blocks
        _blocked(case, pattern, tail(2 * R // 4, 100), rng),        # the last, FULL region ends in 100 empty blocks
        _plain(case, pattern, 2 * R + 5, rng),
        _blocked(case, pattern, np.zeros(0, dtype=np.int64), rng),  # nothing, in blocks
        _plain(case, pattern, cap, rng),
        _blocked(case, pattern, random(cap // 4), rng),     # the whole segment
        _blocked(case, pattern, [1], rng),                  # one block, one point
        _plain(case, pattern, 7, rng),
        _blocked(case, pattern, np.full(3 * R // 4, 15), rng),      # no sentinel at all
    ]


def _flush_and_check(case, segments):
    import torch

    cb, L, w, h = case.cb, case.L, case.w, case.h
    counts, stream = blk.place_segments(L, segments)
    case._write("wave_count", counts)
    case._write("stream", stream)
    row, col = blk.pixels_of(segments)
    start = _start(w * h)
    expected = ref.expected_histogram(start, w, h, np.zeros_like(row), row, col)
    hist = torch.arange(start.size, dtype=torch.int64, device=case.ws.device) * 3 + (1 << 40)
    cb.flush_scatter(case.dims, hist.data_ptr(), case.n_threads, case.ws.data_ptr(), case.bytes)
    torch.cuda.synchronize(hist.device)
    want = torch.from_numpy(expected.view(np.int64)).to(hist.device)
    if not torch.equal(hist, want):
        bad = torch.nonzero(hist != want).reshape(-1)
        first = [(int(i) // w, int(i) % w, int(hist[i] - want[i])) for i in bad[:8]]
        pytest.fail("%d points planted, %d pixels differ; first (row, col, got - expected): %s; wave_count %s; cap %d" % (
            row.size, bad.numel(), first, [hex(int(c)) for c in counts], L.cap))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "%dx%d" % c)
def test_blocked_and_plain_segments_in_one_workspace(cb, monkeypatch, canvas, pattern):
    case = Case(cb, monkeypatch, *canvas)
    assert not case.L.two_level and not case.L.chunked and case.L.n_planes == 1
    _flush_and_check(case, _segments(case, pattern, np.random.default_rng(21)))


@pytest.mark.parametrize("canvas", [(128, 65536), (16512, 128)], ids=lambda c: "%dx%d" % c)
def test_blocked_segments_on_the_general_instance(cb, monkeypatch, canvas):
    """One tile column under more than 256 tile rows, and more than 128 tile columns: the canvases of one level that
    the lean region sort does not take."""
    case = Case(cb, monkeypatch, *canvas)
    assert not case.L.two_level
    _flush_and_check(case, _segments(case, "uniform", np.random.default_rng(22)))
