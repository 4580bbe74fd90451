"""The equalised image restated in Python integers (include/cudabrot_amd.h, "Equalised image") -- test infrastructure only.
The reference project has no such feature, so there is no golden from it: this is the definition written out a second time.

    key(c)   = c for c < 2048, else (s << 10) + (c >> s) with s = floor(log2 c) - 10
    bins[k]  = #{count > 0 with key(count) = k},  lit = sum(bins),  le[k] = sum(bins[j] for j <= k)
    table[0] = 0,  table[k] = cb_tone_value(le[k], lit, gamma)   (the library's: the one floating-point step),
                   but 65535 for the brightest lit key (le[k] = lit) when gamma > 0
    pixel    = table[key(count)]

and the arrays the host and the device suites share (cases())."""

import numpy as np

from exposure_reference import synthetic_histogram

KEYS = 56320
GAMMAS = (1.0, 2.2, 0.5, 0.0, -1.0)
# the values the definition states
KEY_ANCHORS = {0: 0, 1: 1, 2047: 2047, 2048: 2048, 2049: 2048, 4095: 3071, 4096: 3072, (1 << 63) - 1: 55295, (1 << 64) - 1: 56319}


def key(c):
    c = int(c)
    if c < 2048:
        return c
    s = c.bit_length() - 1 - 10
    return (s << 10) + (c >> s)


def lowest_count(k):
    """The smallest counter whose key is k."""
    if k < 2048:
        return k
    s = (k >> 10) - 1
    return (k - (s << 10)) << s


def bins(hist):
    """-> (u64 bins [KEYS], lit, max) of every counter of `hist` taken as one array."""
    a = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    out = [0] * KEYS
    counts, times = np.unique(a, return_counts=True)
    for c, t in zip(counts.tolist(), times.tolist()):
        if c > 0:
            out[key(c)] += t
    return np.array(out, dtype=np.uint64), sum(out), int(a.max()) if a.size else 0


def table(cb, b, gamma):
    """-> (u16 table [KEYS], keys, levels) from bins."""
    b = [int(v) for v in b]
    lit, le, out = sum(b), 0, [0] * KEYS
    for k in range(1, KEYS):
        le += b[k]
        if not b[k]:
            out[k] = out[k - 1]  # an empty bin: the same rank, the same value
        else:
            out[k] = 65535 if le == lit and gamma > 0 else cb.tone_value(le, lit, gamma)  # the full rank is full white
    lit_keys = [k for k in range(KEYS) if b[k]]
    return np.array(out, dtype=np.uint16), len(lit_keys), len({out[k] for k in lit_keys})


def image(cb, hist, gamma):
    """-> (u16 values in the shape of `hist`, lit, keys, levels): one table over all of `hist`."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    b, lit, _ = bins(a)
    t, keys, levels = table(cb, b, gamma)
    counts, where = np.unique(a, return_inverse=True)
    values = np.array([t[key(c)] for c in counts.tolist()], dtype=np.uint16)
    return values[where.reshape(-1)].reshape(a.shape), lit, keys, levels


def key_edges():
    """One counter on each side of every key edge 2^k - 1, 2^k, 2^k + 1 for k = 10 .. 63, among three zeros."""
    values = [v for k in range(10, 64) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)] + [0, 0, 0]
    return np.random.default_rng(2).permutation(np.array(values, dtype=np.uint64)).reshape(11, 15)


def heavy(rng, n, top=60_000):
    """tests/test_gpu_exposure.py's heavy-tailed draw: mostly zeros and small counts, a few near `top`."""
    return np.minimum((rng.pareto(1.2, size=n) * 3).astype(np.uint64), np.uint64(top))


def cases():
    """name -> 2-D array of u64 counters (the colour case: its three planes one above the other, as the image calls take
    them)."""
    rng = np.random.default_rng(13)
    distinct = np.zeros(32 * 80, dtype=np.uint64)
    distinct[:2047] = np.arange(1, 2048, dtype=np.uint64)
    one = np.zeros((5, 7), dtype=np.uint64)
    one[3, 2] = 12345
    colour = np.stack([heavy(rng, 24 * 32, top).reshape(24, 32) for top in (60_000, 700, 1 << 33)])
    return {
        "all_zero": np.zeros((9, 13), dtype=np.uint64),
        "one_lit": one,
        "all_ones": np.ones((17, 19), dtype=np.uint64),
        "distinct_below_2048": rng.permutation(distinct).reshape(32, 80),
        "key_edges": key_edges(),
        "u64_max": np.array([[(1 << 64) - 1, 1, 0]], dtype=np.uint64),
        "heavy_tail": synthetic_histogram(7, 201, 333, 1_000_003),
        "colour_planes": colour.reshape(3 * 24, 32),
    }
