"""TEST INFRASTRUCTURE: planted inputs for the two output stages every image leaves through, the tone map (tonemap.hip)
and the colour stage (color.hip).  Pure numpy.  Each array is built so that one decision of a kernel -- a threshold, a
rank, a bucket boundary, the second trip of a grid-stride loop, a lone tail store -- changes a pixel that is in it.
tests/test_output_planted_host.py shows on the host functions alone that every plant is decisive; the two GPU suites
(tests/test_gpu_tonemap_planted.py, tests/test_gpu_color_planted.py) then compare the device byte for byte.

The tone builders take the host map as a function `value(counts) -> u16 values` (host_map below), so that this module
needs neither the library nor a device.

It also holds what the GPU suites of the whole output stage share (the two above and tests/test_gpu_exposure.py,
test_gpu_equalize.py, test_gpu_density.py): arrays put on the device at an offset, guarded outputs, and the constants a
source file names (the sweep's are counter_sweep.h's)."""

import os
import re

import numpy as np

GAMMAS = (2.2, 1.0, 0.45, 0.0)
DOMAIN_TOPS = (1, 2, 162, 65535, 65536, 1_000_003)
BEYOND_TOPS = ((1 << 24) + 12345, (1 << 37) + 12345, (1 << 53) + 1, (1 << 63) + 5, (1 << 64) - 1)
U64 = np.uint64

# The launches the plants are sized by; each GPU suite checks its half against the source (the_grid_named_here_is_the_code_s).
# tonemap.hip: kSweepThreads lanes, two pixels per lane, the grid capped at 256 * 16 blocks (counter_sweep.h).
TONE_THREADS, TONE_BLOCK_CAP = 256, 256 * 16
TONE_SWEEP = 2 * TONE_BLOCK_CAP * TONE_THREADS
# color.hip: kColorThreads lanes, eight pixels per lane; kLevelBlocksPerPlane blocks per plane in the two level kernels,
# kComposeBlocks in the compose kernel.
COLOR_THREADS, LEVEL_BLOCKS, COMPOSE_BLOCKS = 256, 1024, 4096
LEVEL_SWEEP = LEVEL_BLOCKS * COLOR_THREADS * 8


def u64(values):
    return np.array([int(v) for v in values], dtype=U64)


def source(name):
    """The text of cudabrot_amd/csrc/<name> and the uint32 constants it defines with a literal, {name: value}."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudabrot_amd", "csrc", name)) as f:
        text = f.read()
    return text, {k: int(v) for k, v in re.findall(r"constexpr uint32_t (k\w+) = (\d+);", text)}


# ---- what the GPU suites of the output stage put on the device, and how they look at what comes back ----

GUARD, FILL = 8, 0x5a5a  # u16 on each side of an output


def on_device(values, offset=0, fill=0, spare=0):
    """A u64 array, flat, on cuda:0 `offset` elements into its allocation, `spare` elements behind it, `fill` around it
    -> (tensor that owns it, view)."""
    import torch

    flat = np.array(values, dtype=np.uint64).reshape(-1)  # a copy: the plants are shared and read-only
    base = torch.full((flat.size + offset + spare,), fill, dtype=torch.int64, device="cuda:0")
    view = base[offset:offset + flat.size]
    view.copy_(torch.from_numpy(flat.view(np.int64)))
    torch.cuda.synchronize()
    return base, view


def guarded_output(samples, offset=0):
    """`samples` u16 on cuda:0, GUARD + offset u16 into an allocation filled with FILL -> (the allocation, the output)."""
    import torch

    base = torch.full((GUARD + offset + samples + GUARD,), FILL, dtype=torch.int16, device="cuda:0")
    return base, base[GUARD + offset:GUARD + offset + samples]


def read_guarded(base, samples, offset=0):
    """The output as big-endian samples, after the guards on both sides were seen untouched."""
    host = base.cpu().numpy().view(np.uint16)
    lo = GUARD + offset
    assert np.all(host[:lo] == FILL), "a store in front of the image"
    assert np.all(host[lo + samples:] == FILL), "a store behind the image"
    return host[lo:lo + samples].view(">u2")


# ---- tone map ----


def host_map(cb, top, gamma):
    """The host's map under the maximum `top`, vectorised: counts (<= top) -> u16 values.  cb.set_grayscale_pixels
    takes the maximum of what it is given, so `top` rides along as one more counter."""

    def value(counts):
        a = np.append(np.asarray(counts, dtype=U64).reshape(-1), U64(top)).reshape(1, -1)
        gray, mx, _ = cb.set_grayscale_pixels(a, gamma)
        assert mx == top
        return gray[0, :-1]

    return value


def every_count(top, seed=1):
    """Item 1: every count of [0, top] once, in a seeded order."""
    return np.random.default_rng(seed).permutation(np.arange(top + 1, dtype=U64))


def threshold_edges(value, top):
    """For every output value k in [1, value(top)] the smallest count t in [0, top] with value(t) >= k, by bisection
    over the host map, all k at once -> the distinct t, ascending.  value(t - 1) < k <= value(t) is the loop's
    invariant, so each (t - 1, t) straddles a step of the map by construction."""
    peak = int(value([top])[0])
    k = np.arange(1, peak + 1, dtype=np.int64)
    a = np.zeros(peak, dtype=U64)         # value(0) = 0 < k
    b = np.full(peak, top, dtype=U64)     # value(top) = peak >= k
    while np.any(b - a > U64(1)):
        mid = a + (b - a) // U64(2)
        reach = value(mid).astype(np.int64) >= k
        b = np.where(reach, mid, b)
        a = np.where(reach, a, mid)
    return np.unique(b)


def beyond_the_table(value, top, seed=2):
    """Item 2: t - 1 and t for every distinct edge t, plus 0, 1, top - 1, top (and the two counts around 2^63 where the
    top is above it), shuffled, padded with a zero to an odd length -> (counters, edges)."""
    edges = threshold_edges(value, top)
    extra = [0, 1, top - 1, top] + ([(1 << 63) - 1, 1 << 63] if top > (1 << 63) else [])
    planted = np.concatenate([edges - U64(1), edges, u64(extra)])
    np.random.default_rng(seed).shuffle(planted)
    if planted.size % 2 == 0:
        planted = np.append(planted, U64(0))
    return planted, edges


def heavy_tail(rng, n, below=60_000):
    return np.minimum((rng.pareto(1.2, size=n) * 3).astype(U64), U64(below - 1))


def past_the_first_sweep(value, sweep, top, seed=3):
    """Item 3: sweep + 3 counters, heavy-tailed below 60 000; the last three -- behind a full sweep of the grid -- are 0,
    a threshold edge of the map under `top`, and the sole maximum `top` -> (counters, the edge)."""
    a = heavy_tail(np.random.default_rng(seed), sweep + 3)
    edges = threshold_edges(value, top)
    edge = edges[edges.size // 2]
    assert 60_000 < int(edge) < top
    a[-3:] = u64([0, edge, top])
    return a, int(edge)


def tiny(n):
    """Item 4: n = 1, 2, 3 counters, the maximum last."""
    return u64([5, 2, 3][:n][::-1])


# ---- colour ----

LEVEL_SHAPE = (61, 67)      # odd, and no multiple of the 8 pixels a lane takes
TOP = 65535                 # one pixel of every plane: at gamma 0 the plane's values are then its counts


def stretch_percent(n, rank):
    """A percentage whose rank over n pixels (color_ranks: trunc(n * (P / 100))) is `rank`."""
    p = 100.0 * (rank + 0.5) / n if rank else 0.0
    assert int(float(n) * (p / 100.0)) == rank
    return p


def _draw(rng, lo, hi, count):
    assert lo <= hi and count >= 0
    return np.sort(rng.integers(lo, hi + 1, size=count)).tolist()


def _ordered(pieces, n, nb, nw, black, white):
    """The pieces in ascending order make the plane's multiset: black is then value nb from below, white value nw from
    above (include/cudabrot_amd.h, "Colour image", step 1)."""
    v = [int(x) for piece in pieces for x in piece]
    assert len(v) == n and v == sorted(v) and v[-1] == TOP, (len(v), n)
    assert v[nb] == black and v[n - 1 - nw] == white
    return v, (black, white)


def row_bucket_ends(rng, n, nb, nw):
    """Black on the last value of a high-byte bucket, white on the first value of one; the neighbours across each
    bucket boundary are there too, and the values one rank off differ."""
    return _ordered([_draw(rng, 0x0100, 0x12fd, nb - 1), [0x12fe], [0x12ff], [0x1300], _draw(rng, 0x1301, 0x9ffe, n - nb - nw - 4),
                     [0x9fff], [0xa000], [0xa001], _draw(rng, 0xa002, 0xfffe, nw - 2), [TOP]], n, nb, nw, 0x12ff, 0xa000)


def row_coarse_equality(rng, n, nb, nw):
    """Exactly nb pixels in the buckets below black's, exactly nw in those above white's: the running sum of the
    coarse select EQUALS the rank at the bucket before, and black / white are their buckets' first / last value."""
    return _ordered([_draw(rng, 0x2000, 0x20ff, nb), [0x3105], _draw(rng, 0x3106, 0xc2ef, n - nb - nw - 2), [0xc2f0],
                     _draw(rng, 0xc300, 0xfffe, nw - 1), [TOP]], n, nb, nw, 0x3105, 0xc2f0)


def row_fine_equality(rng, n, nb, nw):
    """As row_coarse_equality, one level down: part of the nb pixels below black share its bucket, so the running sum
    of the FINE select equals the rank left at the low byte before black's.  Likewise above white."""
    return _ordered([_draw(rng, 0x2000, 0x30ff, nb // 2), _draw(rng, 0x3100, 0x3104, nb - nb // 2), [0x3105],
                     _draw(rng, 0x3106, 0xc2ef, n - nb - nw - 2), [0xc2f0], _draw(rng, 0xc2f1, 0xc2ff, nw - nw // 2),
                     _draw(rng, 0xc300, 0xfffe, nw // 2 - 1), [TOP]], n, nb, nw, 0x3105, 0xc2f0)


def row_same_bucket(rng, n, nb, nw):
    """Black and white in one bucket: the fine kernel counts the same pixels into both of its histograms."""
    return _ordered([_draw(rng, 1, 0x54ff, nb // 2), _draw(rng, 0x5500, 0x550f, nb - nb // 2), [0x5510],
                     _draw(rng, 0x5511, 0x55df, n - nb - nw - 2), [0x55e0], _draw(rng, 0x55e1, 0x55ff, nw - nw // 2),
                     _draw(rng, 0x5600, 0xfffe, nw // 2 - 1), [TOP]], n, nb, nw, 0x5510, 0x55e0)


def row_first_and_last_bucket(rng, n, nb, nw):
    """Black in bucket 0 with a non-zero low byte, white in bucket 255."""
    return _ordered([_draw(rng, 0, 0x36, nb), [0x37], _draw(rng, 0x38, 0xff7f, n - nb - nw - 2), [0xff80],
                     _draw(rng, 0xff81, 0xfffe, nw - 1), [TOP]], n, nb, nw, 0x37, 0xff80)


def row_ties(rng, n, nb, nw, run=50):
    """Both ranks inside long runs of one value."""
    r = min(run, nb)
    up = min(run, nw - 1)
    between = n - (nb - r) - (2 * r + 1) - (r + 1 + up) - (nw - up)
    return _ordered([_draw(rng, 0, 0x4443, nb - r), [0x4444] * (2 * r + 1), _draw(rng, 0x4445, 0x8887, between),
                     [0x8888] * (r + 1 + up), _draw(rng, 0x8889, 0xfffe, nw - up - 1), [TOP]], n, nb, nw, 0x4444, 0x8888)


def row_flat(rng, n, nb, nw):
    """White <= black: one value holds both ranks (they cannot cross: B + W < 100)."""
    below, above = nb // 2, max(nw // 2, 1)
    return _ordered([_draw(rng, 0, 4999, below), [5000] * (n - below - above), _draw(rng, 5001, 0xfffe, above - 1), [TOP]],
                    n, nb, nw, 5000, 5000)


def row_no_dark(rng, n, nb, nw):
    """No pixel below 1000: the black level is positive whatever the rank, and its low byte is 0."""
    return _ordered([_draw(rng, 1000, 0x0fff, nb), [0x1000], _draw(rng, 0x1001, 0xeffe, n - nb - nw - 2), [0xefff],
                     _draw(rng, 0xf000, 0xfffe, nw - 1), [TOP]], n, nb, nw, 0x1000, 0xefff)


def row_plain(lowest):
    """For B = W = 0: the levels are the smallest and the largest value."""

    def row(rng, n, nb, nw):
        assert nb == 0 and nw == 0
        return _ordered([[lowest], _draw(rng, lowest, 0xfffe, n - 2), [TOP]], n, 0, 0, lowest, TOP)

    return row


LEVEL_CASES = {
    # name: (nb, nw, the rows of the three planes)
    "bucket_ends_and_equalities": (81, 40, (row_bucket_ends, row_coarse_equality, row_fine_equality)),
    "one_bucket_extremes_ties": (203, 310, (row_same_bucket, row_first_and_last_bucket, row_ties)),
    "flat_bright_equality": (40, 81, (row_flat, row_no_dark, row_coarse_equality)),
    "zero_ranks": (0, 0, (row_plain(1234), row_plain(0x37), row_plain(0))),
}


def level_case(name, seed=4):
    """Item 6 -> {"planes": three u64 arrays LEVEL_SHAPE, "stretch": (B, W), "ranks": (nb, nw), "levels": [(black, white)] * 3}."""
    nb, nw, rows = LEVEL_CASES[name]
    rng = np.random.default_rng(seed)
    n = LEVEL_SHAPE[0] * LEVEL_SHAPE[1]
    planes, levels = [], []
    for row in rows:
        v, lv = row(rng, n, nb, nw)
        planes.append(rng.permutation(np.array(v, dtype=U64)).reshape(LEVEL_SHAPE))
        levels.append(lv)
    return {"planes": planes, "stretch": (stretch_percent(n, nb), stretch_percent(n, nw)), "ranks": (nb, nw), "levels": levels}


def levels_past_the_sweep(sweep, seed=5):
    """Item 7: sweep + 11 pixels per plane, all 30 000 but the last 11 -- seven distinct small values and four distinct
    large ones, 65535 among them, in a seeded order --, with ranks nb = 5 and nw = 2: the levels are the sixth smallest
    and the third largest of the tail, read by the second trip of the level kernels' loops."""
    rng = np.random.default_rng(seed)
    n = sweep + 11
    planes, levels = [], []
    for j in range(3):
        small = rng.choice(np.arange(100 + 3000 * j, 29_000), size=7, replace=False)
        large = np.append(rng.choice(np.arange(31_000 + 3000 * j, TOP), size=3, replace=False), TOP)
        a = np.full(n, 30_000, dtype=U64)
        a[-11:] = rng.permutation(np.concatenate([small, large])).astype(U64)
        planes.append(a.reshape(1, n))
        levels.append((int(np.sort(small)[5]), int(np.sort(large)[-3])))
    return {"planes": planes, "stretch": (stretch_percent(n, 5), stretch_percent(n, 2)), "ranks": (5, 2), "levels": levels}


DECISION_VALUES = (5535, 5536, 15534, 15535, 15536, 25534, 25535, 25536, 35534, 35535, 35536, 45534, 45535, 45536, 65534, 65535)
DECISION_LEVELS = (5535, 65535)
HUE_SHIFTS = (0.0, 0.3, -1.7, 2.0, 1.0 / 6.0)
COMPOSES = (("rgb", 0.0),) + tuple(("hsl", s) for s in HUE_SHIFTS)


def compose_decisions(seed=6):
    """Item 8: with the levels pinned to (5535, 65535) by B = W = 0 the 16 values stretch to 0, 1 and the neighbours of
    1/6, 1/3, 1/2 and 2/3; every triple of them is one pixel, three fillers make n = 4099 (a last group of three)."""
    v = np.array(DECISION_VALUES, dtype=U64)
    grid = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=0).reshape(3, -1)
    order = np.random.default_rng(seed).permutation(grid.shape[1])
    planes = [np.append(grid[j][order], u64([30_000] * 3)).reshape(1, -1) for j in range(3)]
    assert planes[0].size == 4099
    return {"planes": planes, "stretch": (0.0, 0.0), "ranks": (0, 0), "levels": [DECISION_LEVELS] * 3}
