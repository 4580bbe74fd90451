"""The white clip restated in numpy (include/cudabrot_amd.h, "White clip") -- test infrastructure only.  The reference
project has no such feature, so there is no golden from it: this is the definition written out a second time, by sorting.

    lit     = #{count > 0}
    r       = (uint64)((double) lit * (p / 100.0)), clamped to lit - 1 when lit > 0
    white   = the (r + 1)-th largest counter (0 when nothing is lit)
    clipped = #{count > white}
    pixel   = cb_tone_value(min(count, white), white, gamma)

and the arrays the host and the device suites share (CASES), each made to put the rank somewhere awkward."""

import numpy as np

CLIPS = (0.0, 0.1, 1.0, 50.0, 99.0, 99.999999)
GAMMAS = (1.0, 2.2, 0.45, 0.0, -3.0)


def rank(lit, clip):
    if lit == 0:
        return 0
    return min(int(float(lit) * (float(clip) / 100.0)), lit - 1)  # Python's float is the C double; int() truncates


def white_count(hist, clip):
    """-> (white, lit, clipped) of every counter of `hist` taken as one array."""
    a = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    lit = np.sort(a[a > 0])[::-1]
    if lit.size == 0:
        return 0, 0, 0
    white = int(lit[rank(lit.size, clip)])
    return white, int(lit.size), int(np.count_nonzero(a > np.uint64(white)))


def tone_map(cb, hist, gamma, clip):
    """-> (u16 values in the shape of `hist`, white): each distinct count is mapped once through cb.tone_value."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    white, _, _ = white_count(a, clip)
    counts, where = np.unique(np.minimum(a, np.uint64(white)), return_inverse=True)
    values = np.array([cb.tone_value(int(c), white, gamma) for c in counts], dtype=np.uint16)
    return values[where].reshape(a.shape), white


def synthetic_histogram(seed, h, w, top):
    """The heavy-tailed histogram of tests/test_gpu_tonemap.py: mostly small counts, a few near the maximum."""
    rng = np.random.default_rng(seed)
    a = (rng.pareto(1.2, size=(h, w)) * 3).astype(np.uint64)
    a = np.minimum(a, np.uint64(top))
    a[rng.integers(0, h), rng.integers(0, w)] = top
    a[0, :7] = np.arange(7, dtype=np.uint64)
    return a


def planted_histogram():
    """64 x 96 with counters beyond 32 bits: every digit pass of an eight-byte maximum has work."""
    a = synthetic_histogram(11, 64, 96, 1_000_000)
    a[3, 3] = 1 << 32
    a[5, 5] = (1 << 37) + 12345
    a[7, 7] = 1 << 56
    a[9, 9] = (1 << 63) + 1
    return a


def boundary_histogram():
    """1000 lit counters, 10 of value 900 and 990 of value 7, among 200 zeros: at p = 1 the rank r = 10 is the first 7,
    r - 1 = 9 (p = 0.9) the last 900 -- the rank falls exactly between two distinct values."""
    a = np.zeros(1200, dtype=np.uint64)
    a[100:110] = 900
    a[110:1100] = 7
    return np.random.default_rng(3).permutation(a).reshape(30, 40)


BOUNDARY_CLIPS = (0.9, 1.0)  # r = 9 and r = 10 of 1000 lit counters


def cases():
    """name -> 2-D array of u64 counters."""
    return {
        "heavy_tail": synthetic_histogram(7, 201, 333, 1_000_003),
        "all_zero": np.zeros((9, 13), dtype=np.uint64),
        "single_pixel": np.array([[5]], dtype=np.uint64),
        "one_repeated_value": np.full((17, 19), 42, dtype=np.uint64),
        "rank_on_a_boundary": boundary_histogram(),
        "beyond_32_bits": planted_histogram(),
    }
