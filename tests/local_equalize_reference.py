"""The locally equalised image restated in Python integers (include/cudabrot_amd.h, "Locally equalised image"; DESIGN.md
4.28) -- test infrastructure only.  The reference project has no such feature, so there is no golden from it: this is the
definition written out a second time, on sparse bins (a dict key -> count per tile) and Python's unbounded integers.

    ex[i]      = i * w // TX, ey[j] likewise; tile t = j * TX + i is columns [ex[i], ex[i+1]) x rows [ey[j], ey[j+1]) of
                 every plane
    bins_t[k]  = #{count > 0 of tile t with key(count) = k}
    clipped_t  = bins_t for clip_q = 0, else with L = max(1, clip_q * lit_t // (256 * keys_t)) and E = sum(max(0, b - L)):
                 min(b, L) + E // keys_t + (m < E % keys_t) for the m-th lit key
    table_t    = equalize_reference's table of clipped_t; of the sum of all bins, unclipped, for a tile without a lit pixel
    pixel      = the blend of the four tables around it at doubled coordinates, rounded half up

and the arrays and grids the host and the device suites share (cases(), GRIDS, CLIPS)."""

import bisect

import numpy as np

import equalize_reference as eq

GRIDS = [(1, 1), (2, 2), (4, 3), (5, 3), (1, 4), (16, 16)]  # (TX, TY); a case takes those that fit its canvas
CLIPS = (0, 512, 1024)                                      # off, 2 and the binary's default 4, in 1/256ths
GAMMAS = (2.2, 0.0)


def edges(n, t):
    return [i * n // t for i in range(t + 1)]


def centres(n, t):
    e = edges(n, t)
    return [e[i] + e[i + 1] for i in range(t)]


def place(c, p):
    """(i0, i1, a, d) of the doubled coordinate p among the doubled centres c, as the definition words it."""
    t = len(c)
    if t == 1 or p <= c[0]:
        return 0, 0, 0, 1
    if p >= c[t - 1]:
        return t - 1, t - 1, 0, 1
    i0 = max(i for i in range(t) if c[i] <= p)
    return i0, i0 + 1, p - c[i0], c[i0 + 1] - c[i0]


def planes_of(hist):
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


def tile_bins(hist, tx, ty):
    """-> [dict key -> count] per tile, t = j * tx + i."""
    a = planes_of(hist)
    _, h, w = a.shape
    ex, ey = edges(w, tx), edges(h, ty)
    out = []
    for j in range(ty):
        for i in range(tx):
            b = {}
            counts, times = np.unique(a[:, ey[j]:ey[j + 1], ex[i]:ex[i + 1]], return_counts=True)
            for c, n in zip(counts.tolist(), times.tolist()):
                if c > 0:
                    b[eq.key(c)] = b.get(eq.key(c), 0) + n
            out.append(b)
    return out


def dense(bins):
    """The sparse bins of the tiles as the library's array [tiles, KEYS]."""
    out = np.zeros((len(bins), eq.KEYS), dtype=np.uint64)
    for t, b in enumerate(bins):
        for k, n in b.items():
            out[t, k] = n
    return out


def clip(b, clip_q):
    """One tile's sparse bins -> (its clipped bins, E)."""
    if clip_q == 0 or not b:
        return dict(b), 0
    lit, keys = sum(b.values()), len(b)
    limit = max(1, clip_q * lit // (256 * keys))
    excess = sum(max(0, n - limit) for n in b.values())
    return {k: min(b[k], limit) + excess // keys + (1 if m < excess % keys else 0) for m, k in enumerate(sorted(b))}, excess


def curve(cb, b, gamma):
    """The table of sparse bins as (its lit keys ascending, their values): an empty bin has the value of the lit key below
    it, key 0 and everything below the first lit key 0."""
    lit, le, keys, values = sum(b.values()), 0, sorted(b), []
    for k in keys:
        le += b[k]
        values.append(65535 if le == lit and gamma > 0 else cb.tone_value(le, lit, gamma))
    return keys, values


def lookup(table, k):
    keys, values = table
    at = bisect.bisect_right(keys, k)
    return values[at - 1] if at else 0


def image(cb, hist, tx, ty, clip_q, gamma):
    """-> (u16 values in the shape of `hist`, lit, lit_tiles, moved)."""
    a = planes_of(hist)
    planes, h, w = a.shape
    bins = tile_bins(a, tx, ty)
    everything, moved, tables = {}, 0, []
    for b in bins:
        for k, n in b.items():
            everything[k] = everything.get(k, 0) + n
    for b in bins:
        clipped, excess = clip(b, clip_q)
        assert sum(clipped.values()) == sum(b.values()) and all(clipped.values())
        moved += excess
        tables.append(curve(cb, clipped, gamma) if b else None)
    if None in tables:
        shared = curve(cb, everything, gamma)
        tables = [t if t is not None else shared for t in tables]
    columns = [place(centres(w, tx), 2 * x + 1) for x in range(w)]
    rows = [place(centres(h, ty), 2 * y + 1) for y in range(h)]
    out = np.zeros(a.shape, dtype=np.uint16)
    for p in range(planes):
        for y in range(h):
            j0, j1, ay, dy = rows[y]
            for x in range(w):
                c = int(a[p, y, x])
                if c == 0:
                    continue  # table[0] = 0 in every tile
                i0, i1, ax, dx = columns[x]
                k = eq.key(c)
                v00, v10 = lookup(tables[j0 * tx + i0], k), lookup(tables[j0 * tx + i1], k)
                v01, v11 = lookup(tables[j1 * tx + i0], k), lookup(tables[j1 * tx + i1], k)
                num = (dy - ay) * ((dx - ax) * v00 + ax * v10) + ay * ((dx - ax) * v01 + ax * v11)
                out[p, y, x] = (num + dx * dy // 2) // (dx * dy)
    lit_tiles = sum(1 for b in bins if b)
    return out.reshape(np.shape(hist)), sum(everything.values()), lit_tiles, moved


def fits(hist, grid):
    h, w = np.shape(hist)[-2:]
    return grid[0] <= w and grid[1] <= h


def cases():
    """name -> u64 counters [h, w] or [planes, h, w]."""
    rng = np.random.default_rng(29)
    shared = eq.cases()
    half = eq.heavy(rng, 16 * 24, 1 << 20).reshape(16, 24)
    half[:, 12:] = 0                                  # two of every four tiles of a 4 x N grid hold nothing
    crowded = np.full((32, 64), 5, dtype=np.uint64)   # one key holds nearly everything: the clip moves most of it
    crowded[::3, ::5] = rng.integers(1, 4000, size=crowded[::3, ::5].shape).astype(np.uint64)
    crowded[20:, 40:] = 0
    return {
        "all_zero": shared["all_zero"],
        "one_lit": shared["one_lit"],
        "all_ones": shared["all_ones"],
        "key_edges": shared["key_edges"],
        "u64_max": shared["u64_max"],
        "heavy_odd": eq.heavy(rng, 37 * 63, 1 << 36).reshape(37, 63),
        "three_planes": shared["colour_planes"].reshape(3, 24, 32),
        "empty_half": half,
        "crowded": crowded,
    }
