"""The density filter restated in Python integers (include/cudabrot_amd.h, "Density filter") -- test infrastructure only.
The reference project has no such feature, so there is no golden from it: this is the header's text written out a second
time, as the scatter it describes, with math.pow (the C library's pow) for the one floating-point step.

    T[0] = 2^64 - 1;  T[r] = floor(n0 * pow(R / r, 1 / alpha)) for r = 1 .. R;  refused when T[1] >= 2^22
    key    = the sum of a pixel's counters over the planes of its group
    radius = the largest r in 0 .. R with r = 0 or key <= T[r]
    a counter n of a pixel with radius r >= 1 adds n * C(2r, dy + r) * C(2r, dx + r) * 2^(32 - 4r) to acc at (y + dy, x + dx)
    of its own plane, inside the plane only; with radius 0 it is sharp = n at its own place
    out = (sharp << 8) + (acc >> 24)

and the arrays the host and the device suites share (cases), each made to put something awkward in the kernel's way."""

import functools
import math

import numpy as np

MAX_RADIUS = 8
DEFAULT = (4, 0.5, 1)  # (R, alpha, n0)


def thresholds(radius, alpha=0.5, n0=1):
    """T[0 .. R] as Python ints, or None where the definition refuses the parameters."""
    if not (isinstance(radius, int) and 1 <= radius <= MAX_RADIUS and isinstance(n0, int) and 1 <= n0 <= 1 << 20):
        return None
    alpha = float(alpha)
    if not (math.isfinite(alpha) and 1.0 / 16.0 <= alpha <= 4.0):
        return None
    table = [(1 << 64) - 1]
    for r in range(1, radius + 1):
        table.append(int(math.floor(float(n0) * math.pow(float(radius) / float(r), 1.0 / alpha))))
    return None if table[1] >= 1 << 22 else table


def radius_of(key, table):
    return max(r for r in range(len(table)) if r == 0 or key <= table[r])


def density_filter(hist, table, group=1):
    """hist [h, w] or [planes, h, w] -> u64 array of the same shape; None where a counter reaches 2^55."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    cube = a.reshape((1,) + a.shape) if a.ndim == 2 else a
    planes, h, w = cube.shape
    assert group in (1, 3) and planes % group == 0
    if cube.size and int(cube.max()) >= 1 << 55:
        return None
    acc = [[[0] * w for _ in range(h)] for _ in range(planes)]
    sharp = [[[0] * w for _ in range(h)] for _ in range(planes)]
    for g in range(planes // group):
        block = cube[g * group:(g + 1) * group]
        for y, x in zip(*np.nonzero(block.any(axis=0))):
            y, x = int(y), int(x)
            counts = [int(c) for c in block[:, y, x]]
            r = radius_of(sum(counts), table)
            for p, n in enumerate(counts):
                if r == 0:
                    sharp[g * group + p][y][x] = n
                    continue
                rows = acc[g * group + p]
                for dy in range(-r, r + 1):
                    if not 0 <= y + dy < h:
                        continue
                    for dx in range(-r, r + 1):
                        if 0 <= x + dx < w:
                            rows[y + dy][x + dx] += n * math.comb(2 * r, dy + r) * math.comb(2 * r, dx + r) << (32 - 4 * r)
    out = [[[(sharp[p][y][x] << 8) + (acc[p][y][x] >> 24) for x in range(w)] for y in range(h)] for p in range(planes)]
    assert max(max(max(row) for row in plane) for plane in acc) < 1 << 61
    return np.array(out, dtype=np.uint64).reshape(a.shape)


def heavy_tail(seed, h, w, scale=3.0, top=60_000):
    """Mostly zeros and small counts, a few large ones: the counters of a short render."""
    rng = np.random.default_rng(seed)
    return np.minimum((rng.pareto(1.2, size=(h, w)) * scale).astype(np.uint64), np.uint64(top))


def impulse():
    a = np.zeros((9, 9), dtype=np.uint64)
    a[4, 4] = 1
    return a


IMPULSE_ROWS = [[0, 0, 0, 1, 2, 1, 0, 0, 0], [0, 0, 3, 6, 7, 6, 3, 0, 0], [0, 1, 6, 12, 15, 12, 6, 1, 0],
                [0, 2, 7, 15, 19, 15, 7, 2, 0]]  # rows 1 .. 4 of the header's example; 5 .. 7 mirror them, 0 and 8 are zero


def corners_and_edges(h=10, w=13):
    a = np.zeros((h, w), dtype=np.uint64)
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            if (y, x) != (h // 2, w // 2):
                a[y, x] = 1
    return a


def at_the_thresholds(table):
    """Counts T[r] and T[r] + 1 for every r, close enough that their kernels overlap."""
    values = []
    for r in range(1, len(table)):
        values += [table[r], table[r] + 1]
    a = np.zeros((11, 5 * len(values) + 6), dtype=np.uint64)
    for i, v in enumerate(values):
        a[5 + (i % 2), 5 + 5 * i] = v
    return a


def group_of_three():
    """T = 144, 36, 16, 9.  (7, 7, 7): key 21 has radius 2, each plane alone (7 <= 9) would have 4.  (3, 3, 2): key 8, radius
    4 either way.  (0, 40, 0): the key is one plane's, radius 1, and the empty planes of a lit pixel stay empty."""
    a = np.zeros((3, 12, 20), dtype=np.uint64)
    a[:, 5, 5] = 7
    a[:, 6, 8] = (3, 3, 2)
    a[:, 2, 17] = (0, 40, 0)  # out of the reach of the other two
    return a


def four_planes(h=10, w=11):
    a = np.zeros((4, h, w), dtype=np.uint64)
    a[0, h - 1, 4] = 1   # the last row of plane 0
    a[1, 0, 6] = 1       # the first row of plane 1: neither reaches the other
    a[3, 5, 5] = 2
    return a


def huge_beside_one():
    a = np.zeros((8, 8), dtype=np.uint64)
    a[3, 3] = 1 << 54
    a[3, 4] = 1
    return a


def cases():
    """name -> (counters [h, w] or [planes, h, w], group, (R, alpha, n0))."""
    out = {
        "impulse": (impulse(), 1, DEFAULT),
        "corners_and_edges": (corners_and_edges(), 1, DEFAULT),
        "corners_and_edges_r8": (corners_and_edges(), 1, (8, 0.5, 1)),
        "at_the_thresholds": (at_the_thresholds(thresholds(4, 0.4, 16)), 1, (4, 0.4, 16)),
        "at_the_thresholds_r8": (at_the_thresholds(thresholds(8, 0.5, 1)), 1, (8, 0.5, 1)),
        "group_of_three": (group_of_three(), 3, (4, 0.5, 9)),
        "group_of_three_apart": (group_of_three(), 1, (4, 0.5, 9)),
        "four_planes": (four_planes(), 1, DEFAULT),
        "huge_beside_one": (huge_beside_one(), 1, DEFAULT),
        "all_zero": (np.zeros((7, 9), dtype=np.uint64), 1, DEFAULT),
    }
    for params in ((4, 0.5, 4), (8, 0.5, 1), (2, 1.0, 3)):
        out["heavy_tail_%d_%g_%d" % params] = (heavy_tail(5, 23, 31), 1, params)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's answer for a case, computed once per session and shared: do not write to it."""
    hist, group, params = cases()[name]
    out = density_filter(hist, thresholds(*params), group)
    out.setflags(write=False)
    return out
