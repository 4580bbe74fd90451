"""Planted samples: generator states whose FIRST sample is a point the test chose, to the bit, and the finders of the
points worth choosing -- samples that sit on a decision edge of the draw kernels.  Plain Python and numpy on the oracle
(oracle/liboracle.so); neither torch nor pytest.  tests/test_planted_samples_host.py shows on the reference alone that
what this module finds is decisive; tests/test_gpu_planted_samples.py feeds it to the kernels.

THE PLANTING RECIPE.  The generator state is caller-owned memory (six u32 planes x0 .. x4, d on the GPU, the records
of oracle.binding.STATE_DTYPE in the oracle), and XORWOW can be run backwards.  With K = 362437, g(v) = v ^ (v << 4),
f(x) = t ^ (t << 1) where t = x ^ (x >> 2), all mod 2^32:

    output n (n = 1, 2, ...)   o_n  = d + n K + x4_n
    the fifth word             x4_n = g(x4_{n-1}) ^ f(x_{n-1}),   x4_0 = x[4]

and the x_{n-1} of the first four steps are the state's x[0] .. x[3] untouched.  f is a bijection of the 32-bit words
(undo the left shift from bit 0 up, then the right shift from bit 31 down), so for ANY four wanted outputs o_1 .. o_4
and any d and x[4]:

    x4_n = o_n - d - n K,      x[n-1] = f^-1(x4_n ^ g(x4_{n-1}))      n = 1 .. 4.

A coordinate is drawn from two outputs: v = o_a | ((o_b >> 11) << 32), c = (v + 1 - 2^52) * 2^-51 (uniform_double * 4 -
2, every operation exact).  So every double on the 2^-51 grid in (-2, 2] can be planted, 0 and +2 included; -2 cannot (v
would be -1).  The low 11 bits of o_b are free, and so are d and x[4] (plant_states varies them by subsequence, so that
what FOLLOWS the planted sample differs from lane to lane).

THE LIMIT: ONE PLANTED SAMPLE PER SUBSEQUENCE, OF FOUR OUTPUTS OR OF SIX.  Four outputs make one sample of the normal
stream (real, then imag), and four state words take any four outputs whatever d and x[4] are.  A sample of the cell-list
source is six outputs (the entry draw a, b, then x1, x2, y1, y2), and six can be planted as well, by a search
(plant_outputs): the fifth output fixes the last free word, x[4] = f^-1(x4_5 ^ g(x4_4)), the sixth is then a function of d
alone, o_6 = d + 6 K + (g(x4_5) ^ f(x4_1)), and of it only the upper 21 bits matter (the offset draw drops the low 11 of its
second output): one d in 2^21 fits, the search walks all 2^32 if it must and returns an exact state or raises, never a near
one.  Nothing is left free after that, so the second and later samples of a subsequence are the generator's own -- the
oracle, given the same states, follows them too, so a launch of 50 samples per subsequence is still compared bit for bit;
only its first sample is chosen.

The finders bisect the oracle's own predicates over steps of the 2^-51 grid, so what they return is decisive by the
reference's arithmetic, not by a formula about it:

    with_escape_count(N, ray)     a sample whose orc_iterate_mandelbrot count is exactly N
    cardioid_pairs, bulb_pairs    grid neighbours that orc_in_main_cardioid / orc_in_order2_bulb tell apart
    pixel_edge_canvases           canvases on which a given orbit has points where trunc(a / delta) and
                                  trunc(a * RN(1 / delta)) differ (the replay burst's exact-division fallback decides
                                  there), and canvases with an orbit point on, or one ulp off, a canvas edge
    pixel_edge_samples            more samples, on the real axis, with such a point on a given canvas

For the fused multi-channel render the same counts are planted around the edges of several windows at once:

    CHANNEL_SETS, hull            named window sets -- edges on, one past and at the end of a LONG chunk, nested, gapped,
                                  empty, deepest first -- and the one window the fused launch iterates as
    channel_counts, channel_layout   the counts either side of every edge, chunk end and stage start, and their lanes
    fused_model                   per planted count its planes, whether the kernel may record it at once (direct) or
                                  must measure it first, and the counters of the launch, restated from DESIGN.md 4.6

tests/test_planted_channels_host.py shows them decisive on the oracle; tests/test_gpu_planted_channels.py feeds them to
cb_draw_buddhabrot_channels.

The second half of the module does the same for the plotted renders (projected with its steps, Julia, palette, depth,
depth palette, frames, bounded) on THEIR restatement's functions -- plot.step, plot.point, plot.depth_of, plot.slice_of of
tests/plot_reference.py and .c:

    with_end(lib, n, c, **step)   a sample (z_0 under a fixed c) whose orbit escapes at step n under any step of the table
    slice_edges(lib, window)      grid neighbours in c_re that slice_of tells apart, one pair per boundary of the window
    repeating(lib, step, c)       samples whose orbit repeats bit for bit, period 1 and 2, the two on |z|^2 == 4 among them
    c_plane_edges, hologram_canvases   samples on pixel and canvas edges of a dyadic and of an irrational projection
    FILLER                        the sample every family decides at its first step: the lanes not under test are idle
    queue_fills                   the frames render's LDS queue, modelled from the planted lanes' ends

tests/test_planted_plot_host.py shows these decisive on the restatement alone; tests/test_gpu_planted_plot.py and
tests/test_gpu_planted_queue.py feed them to the kernels.

The same finders take the Phoenix step, step = dict(phoenix=(p_re, p_im)), on the Phoenix render's restatement
(tests/phoenix_reference.py and .c: `lib` is then phoenix_reference.load's library): orbit_of, end_of, with_end and
projected_orbit iterate the pair (z, y) from y_0 = 0 with phoenix.step.  Beside them

    ends_found(lib, c, **step)    the ends of ENDS that the rays have under a step, with their samples
    phoenix_cycles(lib, p, c)     samples whose orbit returns to the saved z bit for bit at one chunk and to the saved state
                                  (z, y) at a later one, or never: where the z-only rule and the state rule differ
    PHOENIX_CIRCLE, PHOENIX_REPLAY, PHOENIX_ZEROS   hand-computed orbits: on |z|^2 == 4, for the replay's y_0, with negative zeros

The candidates of PHOENIX_CYCLES beyond the first four are phoenix_cycle_search's: the real axis, where for a p that is a
power of two every operation of the step is a plain rounded product or sum (numpy's doubles do it, 2^16 samples at a time);
like every other plant they count only as far as the restatement's step confirms them.  tests/test_planted_phoenix_host.py shows
these decisive; tests/test_gpu_planted_phoenix.py feeds them to kernels 24 and 25.

The third part is the cell grid of the focused and aimed renders (draw_cells.h; tests/cells_reference.h): six-draw samples
of a cell list, with a reference of the mapping in integers and Fractions that shares no arithmetic with kernels or
restatements, and four-draw samples on the edges of the probe's mask:

    plant_outputs, plant_cell_states   states whose first SIX outputs are chosen
    exact_entry, exact_point           the mapping by the definition: an integer product, a Fraction sum rounded once
    entry_edges, spread_list           entry draws either side of a boundary of j, on lists whose neighbours are far apart
    tie_draws                          offset draws whose exact corner + offset is a tie of the result's format
    interior_edges, map_columns        samples one ulp below a marked cell of the interior map, whose c_re + 2 rounds onto it
    shape_edges_off_the_grid           adjacent doubles across the cardioid's and the bulb's edge, off the 2^-51 grid
    cell_edge_samples, mask_bit        samples on a cell's edge, by the word and the bit of the mask they set

tests/test_planted_cells_host.py shows these decisive; tests/test_gpu_planted_cells.py feeds them to the kernels.
"""

import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import binding as oracle  # noqa: E402

M32 = 0xFFFFFFFF
K = 362437
GRID = 2.0 ** -51
GUARD = 0.5 - 2.0 ** -24          # the replay burst's test on the estimate's fraction (draw_wave.hip, CB_REPLAY_BIN_DIV)


# ---- the generator, backwards ------------------------------------------------------------------------------------------


def _g(v):
    return (v ^ (v << 4)) & M32


def _f(x):
    t = x ^ (x >> 2)
    return (t ^ (t << 1)) & M32


def _f_inverse(y):
    t = 0
    for b in range(32):                       # y = t ^ (t << 1): bit b of t is bit b of y xor bit b - 1 of t
        t |= (((y >> b) ^ ((t >> (b - 1)) if b else 0)) & 1) << b
    x = 0
    for b in range(31, -1, -1):               # t = x ^ (x >> 2): bit b of x is bit b of t xor bit b + 2 of x
        x |= (((t >> b) ^ ((x >> (b + 2)) if b < 30 else 0)) & 1) << b
    return x


def grid_index(c):
    """c as a count of 2^-51 steps; raises unless c is on the grid and in (-2, 2]."""
    n = math.ldexp(float(c), 51)
    if n != int(n) or not -(1 << 52) < n <= (1 << 52):
        raise ValueError("%r is not on the 2^-51 grid in (-2, 2]" % (c,))
    return int(n)


def grid_point(n):
    return math.ldexp(float(n), -51)


def _outputs(c, low):
    v = grid_index(c) + (1 << 52) - 1
    return v & M32, (((v >> 32) << 11) | (low & 0x7FF)) & M32


def first_sample(state):
    """The first sample the oracle draws from a state (which is left as it was)."""
    st = oracle.Xorwow(int(state["d"]), (C.c_uint32 * 5)(*[int(v) for v in state["x"]]))
    re = oracle.lib.orc_uniform_double(C.byref(st)) * 4.0 - 2.0
    im = oracle.lib.orc_uniform_double(C.byref(st)) * 4.0 - 2.0
    return re, im


def plant_state(re, im, d=6615241, x4=5783321, low=0):
    """An oracle state (d, x[5]) whose first sample is exactly (re, im).  d, x4 and the 22 bits of `low` are free."""
    o = _outputs(re, low) + _outputs(im, low >> 11)
    x = [0, 0, 0, 0, x4 & M32]
    before = x[4]
    for n in range(1, 5):
        now = (o[n - 1] - d - n * K) & M32
        x[n - 1] = _f_inverse(now ^ _g(before))
        before = now
    state = np.zeros((), dtype=oracle.STATE_DTYPE)
    state["d"] = d & M32
    state["x"] = x
    assert first_sample(state) == (float(re), float(im)), (re, im, first_sample(state))
    return state


def plant_states(points, salt=0):
    """One state per point, subsequence by subsequence; d, x[4] and the free bits vary with the index (and salt)."""
    out = np.zeros(len(points), dtype=oracle.STATE_DTYPE)
    for k, (re, im) in enumerate(points):
        mix = ((k + 1 + 7919 * salt) * 2654435761) & M32
        out[k] = plant_state(re, im, d=mix ^ 0x2C7F967F, x4=((mix * 40503) ^ (mix >> 7)) & M32 | 1, low=mix >> 9)
    return out


# ---- the reference's step ----------------------------------------------------------------------------------------------


def fma(a, b, c):
    """One rounding: math.fma where Python has it, else the exact rational value rounded to nearest even (finite
    operands).  A zero result takes the sign IEEE gives it."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return a * b + c                       # exact product and sum of zeros: the signs as IEEE has them
    return float(exact)


def mandel_orbit(re, im, n, ship=False):
    """The reference's step (oracle/buddha_oracle.c, mandel_step: one rounding per fma) from z = c, at most n times ->
    (real parts, imag parts, count): the points z_1 .. as IterateAndRecord visits them, the escaping one included and
    last, and IterateMandelbrot's count (the index of the first step with |z|^2 > 4, n if there is none)."""
    r, i = float(re), float(im)
    rs, is_ = [], []
    for k in range(n):
        ii = i * i
        t = fma(r, r, -ii)
        ni = fma(abs(r) + abs(r), abs(i), im) if ship else fma(r + r, i, im)
        r, i = re + t, ni
        rs.append(r)
        is_.append(i)
        if fma(i, i, r * r) > 4:
            return np.array(rs), np.array(is_), k
    return np.array(rs), np.array(is_), n


def real_axis_orbits(c, n):
    """z_1 .. z_n of the real samples c (an array; imag 0): there the step is r <- c + RN(r r) with i = 0, no fused
    operation left, so numpy's doubles do it.  -> [n, len(c)]"""
    c = np.asarray(c, dtype=np.float64)
    r = c.copy()
    out = np.empty((n,) + c.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(n):
            r = c + r * r
            out[k] = r
    return out


def escape_count(re, im, cap):
    return int(oracle.lib.orc_iterate_mandelbrot(float(re), float(im), int(cap)))


def rejected(re, im):
    """What DrawBuddhabrot's shortcut says (either shape)."""
    return bool(oracle.lib.orc_in_main_cardioid(float(re), float(im)) or oracle.lib.orc_in_order2_bulb(float(re), float(im)))


# ---- finders -----------------------------------------------------------------------------------------------------------


def _last_true(pred, lo, hi):
    """pred(lo) and not pred(hi) -> n in [lo, hi) with pred(n) and not pred(n + 1) (or the mirror image for hi < lo)."""
    assert pred(lo) and not pred(hi), (lo, hi)
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


RAYS = {
    "cusp": lambda e: (0.25 + e * GRID, 0.0),      # count ~ pi / sqrt(eps): the parabolic point of the cardioid
    "neck": lambda e: (-0.75, e * GRID),           # count ~ pi / eps: between cardioid and bulb
}
RAY_ENDS = {"cusp": 7 << 49, "neck": 1 << 52}     # the last grid step of either ray: c = 2, and imag = 2 (count 0)


def with_escape_count(n, ray="cusp"):
    """A grid point on the ray whose IterateMandelbrot count is exactly n (n >= 1), outside both shapes of the shortcut.
    The count falls along either ray in bands hundreds of grid steps wide even at 60 000; the bisection ends on the last
    point of band n, next to band n - 1."""
    point = RAYS[ray]
    lo, hi = _last_true(lambda e: escape_count(*point(e), n + 1) >= n, 1, RAY_ENDS[ray])
    c = point(lo)
    assert escape_count(*c, n + 2) == n and escape_count(*point(hi), n + 2) == n - 1, (n, ray, lo)
    assert not rejected(*c)
    return c


def _crossings(pred, rays):
    """rays: (axis, fixed coordinate, inside, outside) -- along the real (0) or the imag (1) axis at the fixed other
    coordinate, from a point where pred holds to one where it does not.  -> [((in), (out))] grid neighbours across the
    edge whose outside point the shortcut does not reject for the other shape either."""
    pairs = []
    for axis, fixed, inside, outside in rays:
        fixed = grid_point(round(math.ldexp(fixed, 51)))            # 0.3 and its like: the grid point next to it
        at = (lambda n: (grid_point(n), fixed)) if axis == 0 else (lambda n: (fixed, grid_point(n)))
        a, b = _last_true(lambda n: pred(*at(n)), grid_index(inside), grid_index(outside))
        if rejected(*at(a)) and not rejected(*at(b)):
            pairs.append((at(a), at(b)))
    return pairs


def cardioid_pairs(n=None):
    """Pairs of grid neighbours (rejected, not rejected) across the edge of orc_in_main_cardioid: both signs of imag,
    imag = 0, the cusp at 1/4 and its surroundings, and -3/4, where cardioid and bulb touch (the point itself is in
    neither: both tests are strict)."""
    tiny, near = 2.0 ** -30, 2.0 ** -12         # (at imag 2^-30 the rounded tests leave no gap between the shapes)
    rays = [(0, 0.0, 0.0, 1.0), (0, tiny, 0.0, 1.0), (0, -tiny, 0.0, 1.0), (0, 2.0 ** -12, 0.0, 1.0),   # the cusp
            (0, 0.0, -0.5, -0.75), (0, near, -0.5, -0.75), (0, -near, -0.5, -0.75)]                       # -3/4
    for y in (0.3, 0.6, 0.125 * 5 + GRID * 12345):
        for s in (1.0, -1.0):
            rays += [(0, s * y, -0.125, 1.0), (0, s * y, -0.125, -0.75)]
    for x in (-0.125, 0.2, -0.7, 0.25 - 2.0 ** -20):
        rays += [(1, x, 0.0, 1.0), (1, x, 0.0, -1.0)]
    pairs = _crossings(lambda re, im: bool(oracle.lib.orc_in_main_cardioid(re, im)), rays)
    return pairs if n is None else pairs[:n]


def bulb_pairs(n=None):
    """The same across the edge of orc_in_order2_bulb (centre -1, radius 1/4)."""
    near = 2.0 ** -12
    rays = [(0, 0.0, -1.0, -1.5), (0, 0.0, -1.0, -0.75), (0, near, -1.0, -0.75), (0, -near, -1.0, -0.75)]
    for y in (0.1, 0.2, 0.25 - 2.0 ** -18):
        for s in (1.0, -1.0):
            rays += [(0, s * y, -1.0, -1.5), (0, s * y, -1.0, -0.75)]
    for x in (-1.0, -1.1, -0.9, -1.25 + 2.0 ** -22):
        rays += [(1, x, 0.0, 1.0), (1, x, 0.0, -1.0)]
    pairs = _crossings(lambda re, im: bool(oracle.lib.orc_in_order2_bulb(re, im)), rays)
    return pairs if n is None else pairs[:n]


# ---- pixel edges -------------------------------------------------------------------------------------------------------


def deltas(box, w, h):
    """The pixel sides as RecomputePixelDeltas makes them (the oracle's own)."""
    d = oracle.make_dims(w, h, box[0], box[1], box[2], box[3])
    return d.delta_real, d.delta_imag


def _axis(z, lo, delta, n, estimate):
    """One coordinate of IncrementPixelCounter: (pixel index, in range), with the quotient or with the estimate alone."""
    z = np.asarray(z, dtype=np.float64)
    a = z - lo
    with np.errstate(over="ignore", invalid="ignore"):
        q = a * (1.0 / np.float64(delta)) if estimate else a / np.float64(delta)
    inside = (z >= lo) & (q < n)                  # for q >= 0, (int) q < n iff q < n
    return np.where(inside, np.trunc(q), -1).astype(np.int64), inside


def pixels(box, w, h, rs, is_, estimate=False):
    """IncrementPixelCounter's pixel of every point -> (col, row, counted)."""
    dr, di = deltas(box, w, h)
    col, okx = _axis(rs, box[0], dr, w, estimate)
    row, oky = _axis(is_, box[2], di, h, estimate)
    return col, row, okx & oky


def histogram(box, w, h, rs, is_, estimate=False):
    col, row, ok = pixels(box, w, h, rs, is_, estimate)
    hist = np.zeros((h, w), dtype=np.uint64)
    np.add.at(hist, (row[ok], col[ok]), 1)
    return hist


def edge_disagreements(box, w, h, rs, is_):
    """The indices of the points that the estimate alone would bin differently from the quotient (counted by at least one
    of the two).  By tests/test_quotient_estimate.py each of them fails the guard, so the kernels' exact division decides
    it -- asserted here as well."""
    cq, rq, okq = pixels(box, w, h, rs, is_)
    ce, re_, oke = pixels(box, w, h, rs, is_, estimate=True)
    differ = (okq | oke) & ((okq != oke) | (cq != ce) | (rq != re_))
    dr, di = deltas(box, w, h)
    for z, lo, d, cols_differ in ((rs, box[0], dr, cq != ce), (is_, box[2], di, rq != re_)):
        est = (np.asarray(z)[differ & cols_differ] - lo) * (1.0 / np.float64(d))
        assert not np.any(np.abs((est - np.floor(est)) - 0.5) < GUARD)
    return np.flatnonzero(differ)


def _edge_hits(z, extent, n, ulps=3):
    """For the coordinates z of an orbit: every lower bound `lo` near z_k - RN(j delta) (a few ulps either way, every
    pixel edge j, every k) for which, on the axis [lo, lo + extent) of n pixels, the guard fails and the two truncations
    differ at z_k.  -> (array of lo, array of k)"""
    z = np.asarray(z, dtype=np.float64)[:, None, None]
    j = np.arange(1, n, dtype=np.float64)[None, :, None]
    lo = z - j * (extent / n)
    lo = lo + np.arange(-ulps, ulps + 1)[None, None, :] * np.spacing(lo)
    delta = ((lo + extent) - lo) / n
    a = z - lo
    q, est = a / delta, a * (1.0 / delta)
    hit = (a >= 0) & (np.trunc(q) != np.trunc(est)) & ~(np.abs((est - np.floor(est)) - 0.5) < GUARD) & (q < n)
    k = np.broadcast_to(np.arange(z.shape[0])[:, None, None], hit.shape)
    return lo[hit], k[hit]


def edge_rate(delta, n):
    """For each pixel side of the array delta: the share of the points on a pixel edge (a = RN(j delta), j < n) or one ulp
    below it whose two truncations differ.  It is a property of the side: of how far RN(1 / delta) is from 1 / delta."""
    sides, back = np.unique(np.asarray(delta, dtype=np.float64), return_inverse=True)
    sides = sides[:, None]
    a = np.arange(1, n, dtype=np.float64)[None, :] * sides
    a = np.concatenate([a, np.nextafter(a, 0.0)], axis=1)
    return (np.trunc(a / sides) != np.trunc(a * (1.0 / sides))).mean(axis=1)[back]


def fma_free_norm(rs, is_):
    """|z|^2 to within an ulp (the choice of canvas edges needs no more)."""
    return np.asarray(rs) ** 2 + np.asarray(is_) ** 2


def pixel_edge_canvases(orbit, w, h, extents=None, limit=4):
    """orbit = (real parts, imag parts) of a planted orbit's recorded points.  -> {kind: [boxes]} with boxes (min_real,
    max_real, min_imag, max_imag) whose pixels are not dyadic:

      "fallback"   some point z_k is binned differently by trunc(a / delta) and by trunc(a * RN(1 / delta)) in its
                   column AND some point in its row, both counted on the canvas: min = z_k - RN(j delta) give or take a
                   few ulps, searched over j, k and a few extents, verified with the oracle's deltas, the best kept;
      "on_min"     an orbit point exactly on min_real, another exactly on min_imag (counted: pixel 0);
      "below_min"  the same points one ulp below the bounds (not counted);
      "on_max"     an orbit point exactly on max_real and one on max_imag: (max - min) / delta truncates to w or to
                   w - 1 -- the oracle says which."""
    rs, is_ = np.asarray(orbit[0], dtype=np.float64), np.asarray(orbit[1], dtype=np.float64)
    if extents is None:
        extents = [(2.6 + 0.0137 * t, 1.4 + 0.0071 * t) for t in range(12)]
    xs, ys = [], []
    for er, ei in extents:
        x, _ = _edge_hits(rs, er, w)
        y, _ = _edge_hits(is_, ei, h)
        x = x[(x <= 0.25) & (x + er >= 1.0)]                    # room for pixel_edge_samples: the real axis right of the
        y = y[(y <= -0.1) & (y + ei >= 0.1)]                    # cusp, imag = 0 well inside
        xs += [(r, float(v), float(v + er)) for r, v in zip(edge_rate(((x + er) - x) / w, w), x)]
        ys += [(r, float(v), float(v + ei)) for r, v in zip(edge_rate(((y + ei) - y) / h, h), y)]
    xs.sort(reverse=True)                                       # the pixel sides that disagree most often first
    ys.sort(reverse=True)
    found = []
    for (_, x0, x1), (_, y0, y1) in zip(xs, ys):
        box = (x0, x1, y0, y1)
        idx = edge_disagreements(box, w, h, rs, is_)
        cq, rq, _ = pixels(box, w, h, rs, is_)
        ce, re_, _ = pixels(box, w, h, rs, is_, estimate=True)
        if np.any(cq[idx] != ce[idx]) and np.any(rq[idx] != re_[idx]):
            found.append(box)
        if len(found) == limit:
            break
    out = {"fallback": found}
    er, ei = extents[0]
    # among the points before the orbit's last sixteen, which take it away: the rest stays on the canvas with them
    bounded = (np.arange(len(rs)) < max(len(rs) - 16, 1)) & (fma_free_norm(rs, is_) <= 4.0)
    kx, ky = int(np.argmin(np.where(bounded, rs, np.inf))), int(np.argmin(np.where(bounded, is_, np.inf)))
    x, y = float(rs[kx]), float(is_[ky])
    out["on_min"] = [(x, x + er, y, y + ei)]
    xb, yb = float(np.nextafter(x, np.inf)), float(np.nextafter(y, np.inf))
    out["below_min"] = [(xb, xb + er, yb, yb + ei)]
    kx, ky = int(np.argmax(np.where(bounded, rs, -np.inf))), int(np.argmax(np.where(bounded, is_, -np.inf)))
    x, y = float(rs[kx]), float(is_[ky])
    out["on_max"] = [(x - er, x, y - ei, y)]
    return out


def pixel_edge_samples(box, w, n, max_iter, min_iter, depth=40, spread=24):
    """Up to n DISTINCT samples on the real axis, right of the cusp, each recorded under (max_iter, min_iter) and each with
    an orbit point whose column the estimate alone would get wrong on this canvas.  For a pixel edge j and an orbit index
    k the sample with z_k = min_real + RN(j delta) is bisected (z_k rises with c there) and its grid neighbours are kept
    where they verify.  The row of these points is that of imag = 0, which must lie on the canvas."""
    dr, _ = deltas(box, w, 1)
    lo_c, hi_c = grid_index(with_escape_count(max_iter - 1, "cusp")[0]), grid_index(with_escape_count(min_iter, "cusp")[0])
    ends = real_axis_orbits(np.array([grid_point(lo_c), grid_point(hi_c)]), depth)
    samples = []
    for k in range(depth - 1, 0, -1):
        edges = box[0] + np.arange(1, w) * dr
        edges = edges[(edges > ends[k, 0]) & (edges < ends[k, 1]) & (edges < 2.0)]
        if not len(edges):
            continue
        a, b = np.full(len(edges), lo_c, dtype=np.int64), np.full(len(edges), hi_c, dtype=np.int64)
        while np.any(b - a > 1):
            mid = (a + b) // 2
            below = real_axis_orbits(mid * GRID, k + 1)[k] < edges
            a, b = np.where(below, mid, a), np.where(below, b, mid)
        near = (a[:, None] + np.arange(-spread, spread + 1)[None, :]).reshape(-1)
        near = np.unique(near[(near >= lo_c) & (near <= hi_c)])
        z = real_axis_orbits(near * GRID, k + 1)[k]
        cq, _ = _axis(z, box[0], dr, w, False)
        ce, _ = _axis(z, box[0], dr, w, True)
        for g in near[cq != ce]:
            c = grid_point(int(g))
            if c not in samples and min_iter <= escape_count(c, 0.0, max_iter) < max_iter and not rejected(c, 0.0):
                samples.append(c)
        if len(samples) >= n:
            break
    return [(c, 0.0) for c in samples[:n]]


# ---- the cases both suites use -----------------------------------------------------------------------------------------

CHUNK, HEAD_STEPS, MID_MIN = 60, 4, 12            # kernels.h kChunk; draw_wave.hip kHeadSteps, plan_stages' kMidMin

WIDE_WINDOWS = [(1234, 20), (2000, 20), (20000, 20)]                                # draw_wide_kernel's usual split
PROBE_WINDOWS = [(3000, 1000), (2999, 1007), (60000, 45000), (60007, 45011)]        # min_iter inside the LONG stage


def stage_plan(max_iter, min_iter):
    """plan_stages (draw_wave.hip) restated -> (long_start, tail_start): the first iteration of the LONG stage, and of an
    orbit's last, shorter chunk (max_iter where the LONG stage is whole chunks: no tail chunk).  (None, None): HEAD and
    MID do all of it, there is no LONG stage -- max_iter lies inside them (a hull like (16, 0) of the channel sets)."""
    mid = 16 if min_iter <= HEAD_STEPS + MID_MIN else MID_MIN + (min_iter - HEAD_STEPS - MID_MIN) % CHUNK
    long_start = HEAD_STEPS + mid
    if max_iter <= long_start:
        return None, None
    return long_start, max_iter - (max_iter - long_start) % CHUNK


def window_counts(max_iter, min_iter):
    """The escape counts worth planting for a window: two either side of each decision -- min_iter (too fast / recorded),
    max_iter (recorded / never escaped) --, the first LONG chunk's first and last steps and the next chunk's first two, and
    the steps either side of the tail chunk's start."""
    long_start, tail_start = stage_plan(max_iter, min_iter)
    counts = {max_iter + k for k in (-2, -1, 0, 1)} | {min_iter + k for k in (-2, -1, 0, 1)}
    counts |= {long_start + k for k in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1)} | {tail_start + k for k in (-1, 0, 1)}
    return sorted(n for n in counts if 1 <= n <= max_iter + 1)


def window_samples(max_iter, min_iter):
    """[(count, (re, im))]: every count of window_counts on both rays."""
    return [(n, with_escape_count(n, ray)) for n in window_counts(max_iter, min_iter) for ray in ("cusp", "neck")]


def expected_fate(count, max_iter, min_iter):
    """The oracle counter that a sample of this escape count adds to (DrawBuddhabrot, cudabrot.cu:400-411)."""
    return "never_escaped" if count >= max_iter else ("too_fast" if count < min_iter else "recorded")


DULL = [(0.0, 0.0), (2.0, 2.0), (-1.0, 0.0), (1.5, -1.5)]     # in the cardioid, gone at once, in the bulb, gone at once


def layout(deep, threads, shape):
    """One planted first sample per subsequence: the deep samples `deep` cycled through "every" lane, or given to
    subsequences 0 and 63 only ("ends": lanes 0 and 63 of the first wave), or to subsequence 64 + 5 only ("b_only": in
    draw_wide_kernel generator B of lane 5 of the first wave, whose generator A is subsequence 5) -- the rest draw dull
    samples that never reach the LONG stage."""
    if shape == "every":
        return [deep[k % len(deep)] for k in range(threads)]
    points = [DULL[k % len(DULL)] for k in range(threads)]
    for n, k in enumerate({"ends": (0, 63), "b_only": (64 + 5,)}[shape]):
        points[k] = deep[n % len(deep)]
    return points


def pixel_edge_cases(w, h, count=1233, max_iter=1234, min_iter=20, samples=24):
    """The pixel-edge inputs both suites use -> (base, {"fallback": [(box, [samples])], "on_min": [box], "below_min":
    [box], "on_max": [box]}): the neck sample of the given escape count, pixel_edge_canvases for its orbit, and for each
    fallback canvas the base sample followed by pixel_edge_samples' real ones."""
    base = with_escape_count(count, "neck")
    rs, is_, _ = mandel_orbit(*base, max_iter)
    canvases = pixel_edge_canvases((rs, is_), w, h)
    canvases["fallback"] = [(box, [base] + pixel_edge_samples(box, w, samples, max_iter, min_iter))
                            for box in canvases["fallback"]]
    return base, canvases


# ---- the cases both channel suites use ---------------------------------------------------------------------------------
#
# The fused multi-channel render (cb_draw_buddhabrot_channels): windows [(max_iter, min_iter)], plane j is
# what a run of its own with window j adds.  tests/test_planted_channels_host.py shows on the oracle alone that the sets
# and the planted counts below are decisive; tests/test_gpu_planted_channels.py feeds them to the kernel.  With kChunk = 60
# and a hull min of 20 the LONG stage starts at 20 and its chunks at 20 + 60 i.

CHANNEL_SETS = {
    # every edge is a chunk's first index and there is no tail chunk: every accepted orbit is direct, none is measured
    "edges_on_chunk_starts": [(140, 20), (620, 140), (2540, 620)],
    # the chunk [140, 199] holds the edge 141; the tail chunk is one step long
    "edges_one_past_a_start": [(141, 20), (621, 141), (2541, 621)],
    # the edge is a chunk's last index, k_hi; the tail chunk is 59 steps long
    "edges_on_a_chunk_s_last_index": [(199, 20), (679, 199), (2599, 679)],
    "recipe_small": [(100, 20), (600, 100), (2500, 600)],                         # the colour recipe's shape at small depth
    # an orbit is in 4, 2 or 1 planes; the first and the last window are identical, so a shallow orbit's passes go through
    # every tag (with the outermost window twice, as first proposed, the counts would be 4, 3 and 2: never a single plane)
    "nested_four": [(150, 20), (800, 20), (3000, 20), (150, 20)],
    # the recipe's own order, deepest first, and two gaps: an orbit in a gap is measured and then counted too_fast
    "recipe_deepest_first": [(60000, 45000), (8000, 1000), (500, 20)],
    "gap_min_below_head": [(60, 5), (700, 300)],                                  # accepted in HEAD / MID: no chunk is known
    "shallow": [(10, 0), (16, 5)],                                                # no LONG stage at all, min_iter 0
    "empty_windows_among_others": [(500, 50), (100, 200), (300, 300)],            # planes 1 and 2 stay zero
    # the probe path: long_start 40, the edge 1007 lies inside the chunk [1000, 1059], 2999 in the tail chunk
    "hull_min_deep": [(3000, 1000), (2999, 1007)],
}


def hull(windows):
    """(max_iter, min_iter) of the one run the fused launch iterates as (cb_draw_buddhabrot_channels): the largest max
    and the smallest min of the windows, empty ones included."""
    return max(m for m, _ in windows), min(c for _, c in windows)


def chunk_of(k, long_start):
    """(first, last) index of the 60-step LONG chunk that holds iteration k >= long_start."""
    first = long_start + (k - long_start) // CHUNK * CHUNK
    return first, first + CHUNK - 1


def channel_counts(windows):
    """The escape counts worth planting for a set of windows: two either side of every window's min and max; the first
    and last index of the LONG chunk that holds each of these edges and of the chunks before and after it; the steps
    either side of the LONG stage's start and of the tail chunk's; and of the hull's max.  From 1 (no grid point of the
    rays has count 0) to the hull's max + 1."""
    top, low = hull(windows)
    long_start, tail_start = stage_plan(top, low)
    counts = {top + k for k in (-1, 0, 1)}
    for m, c in windows:
        for edge in (m, c):
            counts |= {edge + k for k in (-2, -1, 0, 1)}
            if long_start is not None and edge >= long_start:
                first, _ = chunk_of(edge, long_start)
                for start in (first - CHUNK, first, first + CHUNK):
                    if start >= long_start:
                        counts |= {start, start + CHUNK - 1}
    if long_start is not None:
        counts |= {long_start + k for k in (-1, 0, 1)} | {tail_start + k for k in (-1, 0, 1)}
    return sorted(n for n in counts if 1 <= n <= top + 1)


_planted = {}


def channel_samples(windows):
    """[(count, (re, im))]: every count of channel_counts on both rays (found once per count and ray)."""
    out = []
    for n in channel_counts(windows):
        for ray in ("cusp", "neck"):
            if (n, ray) not in _planted:
                _planted[n, ray] = with_escape_count(n, ray)
            out.append((n, _planted[n, ray]))
    return out


def fused_model(windows, counts):
    """What a fused launch does with samples of the given escape counts (None: a sample the shortcut rejects), by DESIGN.md
    4.6 and the header's "Counters of a fused launch" -> {"samples": [(planes, how)], "planes": per plane the number of
    orbits recorded into it, rejected, never_escaped, too_fast, recorded, replay_steps}.

    planes: the tuple of the j with min_j <= k < max_j.  how: None for a sample the hull run does not accept (rejected,
    k >= hull max: never escaped, k < hull min: too fast); else "direct" or "measured".  An accepted orbit is DIRECT when
    the LONG stage knows the 60-step chunk it escaped in -- a full chunk [long_start + 60 i, + 60) that ends at or before
    tail_start: not an escape in HEAD or MID, not one in the last, shorter chunk --, no window begins or ends inside that
    chunk (an edge e, the min or max of any window, an empty one too, with first < e <= last: an edge ON the first index
    leaves the whole chunk on one side), and it lands in at least one window.  Every other accepted orbit is MEASURED:
    replayed once without recording, for its exact index.  recorded: accepted and in some window; too_fast: escaped and in
    none; replay_steps: k + 1 steps per pass, one pass per plane and one more where measured."""
    top, low = hull(windows)
    long_start, tail_start = stage_plan(top, low)
    edges = {e for w in windows for e in w}
    out = {"samples": [], "planes": [0] * len(windows), "rejected": 0, "never_escaped": 0, "too_fast": 0, "recorded": 0,
           "replay_steps": 0}
    for k in counts:
        if k is None:
            out["rejected"] += 1
            out["samples"].append(((), None))
            continue
        if k >= top:
            out["never_escaped"] += 1
            out["samples"].append(((), None))
            continue
        planes = tuple(j for j, (m, c) in enumerate(windows) if c <= k < m)
        out["recorded" if planes else "too_fast"] += 1
        if k < low:
            assert not planes
            out["samples"].append(((), None))
            continue
        measured = True
        if long_start is not None and long_start <= k < tail_start:
            first, last = chunk_of(k, long_start)
            measured = any(first < e <= last for e in edges) or not planes
        for j in planes:
            out["planes"][j] += 1
        out["replay_steps"] += (k + 1) * (len(planes) + (1 if measured else 0))
        out["samples"].append((planes, "measured" if measured else "direct"))
    return out


def recorded_by_windows(windows, per_window, of_hull):
    """The fused run's `recorded` from the oracle's separate runs: per_window[j] and of_hull are the `recorded` of window j
    and of the hull window.  Windows that share no index (adjacent, gapped, empty): the sum; windows whose union is the
    whole hull (nested in the outermost, or overlapping end to end): the hull's, which is the outermost window's where
    there is one.  Where both hold they must agree; a set for which neither holds has no rule here."""
    top, low = hull(windows)
    spans = sorted((c, m) for m, c in windows if c < m)
    disjoint = all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    reach = low
    for c, m in spans:
        reach = max(reach, m) if c <= reach else reach
    covers = bool(spans) and spans[0][0] == low and reach == top
    assert disjoint or covers, windows
    if disjoint and covers:
        assert sum(per_window) == of_hull, (windows, per_window, of_hull)
    return sum(per_window) if disjoint else of_hull


_counts = {}


def counts_of(points, cap, ship=False):
    """The escape count of every point as fused_model takes it: None where the shortcut rejects the sample (never, under
    the Burning Ship step, which has no shortcut), else the oracle's IterateMandelbrot count up to `cap` (of its
    RENDER_BURNING_SHIP build where asked).  Once per point."""
    out = []
    oracle.lib.orc_set_burning_ship(1 if ship else 0)
    try:
        for p in points:
            key = (p, cap, ship)
            if key not in _counts:
                _counts[key] = None if (not ship and rejected(*p)) else escape_count(p[0], p[1], cap)
            out.append(_counts[key])
    finally:
        oracle.lib.orc_set_burning_ship(0)
    return out


def channel_layout(windows, threads):
    """One planted first sample per subsequence, every sample of channel_samples among them and the three fates in
    balance -> (samples, points).  Most planted counts are recorded ones, so every fourth lane cycles through the samples
    that never escape (counts of the hull's max and beyond), the lane after it through those that escape in no window
    (where the set has any), and the other two through all samples in turn."""
    samples = channel_samples(windows)
    top, _ = hull(windows)
    model = fused_model(windows, [n for n, _ in samples])
    never = [c for n, c in samples if n >= top]
    nowhere = [c for (n, c), (planes, _) in zip(samples, model["samples"]) if n < top and not planes]
    everyone = [c for _, c in samples]
    points, turn = [], 0
    for k in range(threads):
        if k % 4 == 0:
            points.append(never[(k // 4) % len(never)])
        elif k % 4 == 1 and nowhere:
            points.append(nowhere[(k // 4) % len(nowhere)])
        else:
            points.append(everyone[turn % len(everyone)])
            turn += 1
    assert set(everyone) <= set(points), "more planted samples than lanes for them"
    return samples, points


def occupancy_counts(windows):
    """The planted counts of the occupancy layouts: for every kind of accepted orbit that channel_counts has -- its planes
    and whether it is direct or measured -- the deepest count of that kind, and the hull's max (an orbit that never
    escapes)."""
    counts = channel_counts(windows)
    model = fused_model(windows, counts)
    deepest = {}
    for n, (planes, how) in zip(counts, model["samples"]):
        if how is not None:
            deepest[planes, how] = n
    return sorted(set(deepest.values()) | {hull(windows)[0]})


# ---- the plotted renders: plants found on the restatement's own functions (tests/plot_reference.py, .c) ---------------------
#
# Everything below takes `lib`, plot_reference.load's library, and decides by plot.step, plot.point, plot.depth_of and
# plot.slice_of alone.  A STEP is the keyword arguments of plot.step (degree, ship, formula); c None: the sample is c and
# z_0, else c is fixed and the sample is z_0 (a Julia render).  An orbit's `end` is the step whose point escapes (the
# scheduler's l.end; the reference's escape index k is end - 1).

import phoenix_reference as phoenix  # noqa: E402
import plot_reference as plot  # noqa: E402

ROUND, MANDELBROT = 12, {}                         # draw_rounds.h kRound; the reference's own step


def header_value(name):
    """The integer include/cudabrot_amd.h defines under the name."""
    import re

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cudabrot_amd.h")) as f:
        m = re.search(r"^#define %s\s+(\S+)" % re.escape(name), f.read(), re.M)
    assert m, name
    return int(m.group(1), 0)


# every formula code and every Multibrot degree the header defines, by the name of the command line or "power_D"
FORMULA_CODES = range(header_value("CB_FORMULA_TRICORN"), header_value("CB_FORMULA_MAX") + 1)
DEGREES = range(header_value("CB_POWER_MIN"), header_value("CB_POWER_MAX") + 1)
assert sorted(plot.NAMES.values()) == list(FORMULA_CODES)
FORMULA_STEPS = {name: dict(formula=code) for name, code in sorted(plot.NAMES.items(), key=lambda kv: kv[1])}
POWER_STEPS = {"power_%d" % d: dict(degree=d) for d in DEGREES}

# The filler: a sample every family decides on the spot.  From z_0 = 2 + 2i the first step of every step there is, under any
# c in [-2, 2]^2, lands at |z_1|^2 >= 36: `end` is 1, so it is too fast under any min_iter >= 1 and, in a bounded render,
# an escaper.  (0, 0) is decided sooner still under the Mandelbrot step on a sampled c -- rejected --, but is an orbit that
# never escapes under every other family.  plot_host checks both on the restatement.
FILLER = (2.0, 2.0)


def orbit_of(lib, sample, n, c=None, **step):
    """z_1 .. of the sample under the restatement's step, at most n points, the escaping one included and last ->
    (points [(r, i)], end or None where none of the n escapes)."""
    cr, ci = sample if c is None else c
    r, i = float(sample[0]), float(sample[1])
    p, yr, yi = step.get("phoenix"), 0.0, 0.0
    points = []
    for k in range(1, n + 1):
        if p is None:
            r, i, m = plot.step(lib, cr, ci, r, i, **step)
        else:                                      # the state is the pair (z, y), y_0 = 0; y is never a point
            r, i, yr, yi, m = phoenix.step(lib, cr, ci, p[0], p[1], r, i, yr, yi)
        points.append((r, i))
        if m > 4.0:
            return points, k
    return points, None


def end_of(lib, sample, cap, c=None, **step):
    """The sample's `end` under the restatement's step, None if none of z_1 .. z_cap escapes."""
    return orbit_of(lib, sample, cap, c, **step)[1]


# rays from a point that never escapes to one that escapes at once; the count falls along them in wide bands near the start
SAMPLED_RAYS = [
    lambda e: (0.25 + e * GRID, 0.0),              # the cusp, where every step of the table is the reference's (z > 0 real)
    lambda e: (0.25 + e * GRID, 2.0 ** -12),       # beside it: the imaginary part and the cross term take part
    lambda e: (0.25 + 2.0 ** -3 + e * GRID, 0.0),  # degree 3 on the real axis: bounded up to 2 / sqrt(27) = 0.3849...
]
FIXED_C = (0.25, 0.0)                              # a Julia set with a parabolic point: z_0 = 1/2 stays, z_0 > 1/2 crawls away
FIXED_RAYS = [lambda e: (0.5 + e * GRID, 0.0), lambda e: (0.5 + e * GRID, 2.0 ** -12)]
RAY_LAST = 3 << 50                                 # every ray ends at or before real part 2 (e GRID = 1.5)


def ray_from(start, direction):
    """The ray start + e GRID direction: a start on the grid and a direction of integers keep every point on it."""
    return lambda e: (start[0] + e * GRID * direction[0], start[1] + e * GRID * direction[1])


# The Phoenix step (step = dict(phoenix=(p_re, p_im)), on phoenix_reference.load's library).  A sampled c next to 0 is z_0
# too and y_0 = 0, so the orbit stays next to 0 for any p with |sqrt(p)| < 1 and leaves it slowly for the others: rays from
# c = 0 up the imaginary axis and along the real one have every band for p = (-1/2, 0) and (0.3, -0.4), and bands up to 61
# at the bounds p = +-(2, 2).  PHOENIX_C is tests/test_gpu_phoenix.py's fixed c of p = (-1/2, 0); the rays of the Julia
# renders start at z_0 = 1/2, which escapes within a few steps there, so these start at a z_0 inside that set (it does
# not escape in 1000 steps).  They leave the sample plane before they end; what is returned is on the grid or refused.
PHOENIX_SAMPLED_RAYS = [ray_from((0.0, 0.0), (0, 1)), ray_from((0.0, 0.0), (1, 0)), ray_from((0.0, 2.0 ** -12), (0, 1))]
PHOENIX_C = (0.56667, 0.0)
PHOENIX_FIXED_RAYS = [ray_from((-0.5625, 0.84375), (0, 1)), ray_from((-0.5625, 0.84375), (1, 0))]


# The formula steps differ from the reference's step, and from one another, by signs and absolute values of z_re, z_im and
# t = z_re^2 - z_im^2 (include/cudabrot_amd.h, "Formula step"): on the rays above, where all three stay positive, the five
# are two maps.  These rays start left of the imaginary axis and cross |z_im| > |z_re|; with_end takes a formula's plant
# from them and keeps it only where steps_told_apart says that the orbit up to `end` is another one under every other
# step of EVERY_STEP.  One step cannot separate all seven: z_1 has one of two real parts (t or |t|) and one of two
# imaginary parts (+-|2 z_re z_im| + c_im), so a plant of end 1 tells four classes apart, the most there are.
# Another orbit under every other step still leaves an absolute value unproven where no other step differs by it alone:
# buffalo's |z_im| matters only where z_im < 0, and from a c_im > 0 its z_im never is.  So a plant of end > 1 must also
# have, among the points z_0 .. z_{end-1} that are stepped from, one with t < 0, one with z_re < 0 and one with z_im < 0 (the
# other coordinate not 0): signs_seen.  The last two rays, just below the real axis and leftwards, are buffalo's.
FORMULA_RAYS = [ray_from((-1.0, 2.0 ** -12), (0, 1)), ray_from((-1.0, 2.0 ** -12), (1, -1)),
                ray_from((-1.0, -2.0 ** -12), (-1, 0)), ray_from((-1.0, -2.0 ** -20), (-1, 0))]
EVERY_STEP = [MANDELBROT, dict(ship=True)] + list(FORMULA_STEPS.values())


def steps_told_apart(lib, sample, n):
    """How many different orbits z_1 .. z_n (each cut at its escape) the sampled c has under the steps of EVERY_STEP."""
    return len({tuple(orbit_of(lib, sample, n, **st)[0]) for st in EVERY_STEP})


def signs_seen(lib, sample, end, **step):
    """(t < 0, z_re < 0, z_im < 0) each at some point of z_0 .. z_{end-1} under the step, the other coordinate not 0."""
    points = [sample] + orbit_of(lib, sample, end, **step)[0][:-1]
    return (any(r * r < i * i for r, i in points), any(r < 0 and i != 0 for r, i in points),
            any(i < 0 and r != 0 for r, i in points))


def told_apart_at(end):
    """What steps_told_apart must give for a formula's plant: every step another orbit, or the four classes of one step."""
    return 4 if end == 1 else len(EVERY_STEP)


def with_end(lib, end, c=None, ray=None, **step):
    """A grid sample whose orbit escapes exactly at step `end` (>= 1) under the restatement's step: the last point of the
    band `end` along a ray, next to the band end - 1; z_0 where c is fixed.  The rays are tried in turn (or the one given)
    and what is returned is verified, not assumed."""
    rays = (FIXED_RAYS if c is not None else SAMPLED_RAYS) if ray is None else [ray]
    if ray is None and c is None and (step.get("ship") or step.get("formula")):
        rays = [rays[1], rays[0], rays[2]]          # off the axis first: on it these steps are the reference's own
    if ray is None and step.get("phoenix") is not None:
        rays = (PHOENIX_FIXED_RAYS if c is not None else PHOENIX_SAMPLED_RAYS) + rays
    decisive = ray is None and c is None and bool(step.get("formula"))
    if decisive:
        rays = FORMULA_RAYS + rays
    for point in rays:
        def lasts(e):
            got = end_of(lib, point(e), end, c, **step)
            return got is None or got >= end
        if end == 1:
            lo = RAY_LAST
        elif lasts(1) and not lasts(RAY_LAST):
            lo, _ = _last_true(lasts, 1, RAY_LAST)
        else:
            continue
        sample = point(lo)
        if c is not None and step.get("phoenix") is not None and max(abs(sample[0]), abs(sample[1])) > 2.0:
            continue                                # a Phoenix ray's last point, for end 1, is beyond the sample plane
        grid_index(sample[0]), grid_index(sample[1])
        if decisive and steps_told_apart(lib, sample, end) != told_apart_at(end):
            continue
        if decisive and end > 1 and not all(signs_seen(lib, sample, end, **step)):
            continue
        if end_of(lib, sample, end + 2, c, **step) == end and (c is not None or step or not rejected(*sample)):
            return sample
    raise ValueError("no ray has a sample with end %d under %r, c %r" % (end, step, c))


def ends_found(lib, c=None, ends=None, **step):
    """[(end, sample)] of the ends of the list (ENDS) that with_end finds under the step: where the rays have no band for an
    end -- at the bounds of the Phoenix parameter the orbits leave too fast for the long ones -- it is left out, and the
    caller says which ends it needs."""
    found = []
    for end in (ENDS if ends is None else ends):
        try:
            found.append((end, with_end(lib, end, c, **step)))
        except ValueError:
            pass
    return found


def slice_edges(lib, window, around=1 << 20):
    """window = (min, max, N) of a depth along the row `cr`, where the depth of every point of an orbit is the sample's
    c_re exactly.  -> {"pairs": [(j, below, above, slice below, slice above)], "disagree": [(c_re, slice, other)]}:
    for every boundary j = 0 .. N whose two sides are both on the grid (min = -2 has nothing plantable below it) the grid
    neighbours in c_re that plot.slice_of tells apart (None: outside the window), bisected over grid steps around min + j
    delta; and, for a window whose delta is no power of two, the grid points within 64 steps of a boundary at which
    trunc(fd / delta) -- plot.slice_of's, asserted -- and trunc(fd * RN(1 / delta)) differ, if the grid has any."""
    lo, hi, n = window
    delta = (hi - lo) / float(n)

    def slice_at(g):
        return plot.slice_of(lib, plot.depth_of(lib, "cr", 0.0, 0.0, grid_point(g), 0.0), lo, hi, n)

    def rank(g):                                   # None (below), 0 .. N - 1, None (above) as -1 .. N
        s = slice_at(g)
        return s if s is not None else (-1 if grid_point(g) < lo + delta / 2 else n)

    out = {"pairs": [], "disagree": []}
    for j in range(n + 1):
        centre = int(round(math.ldexp(lo + j * delta, 51)))
        a, b = max(centre - around, 1 - (1 << 52)), min(centre + around, 1 << 52)
        if not (rank(a) < j <= rank(b)):
            continue                               # nothing plantable on one side
        a, b = _last_true(lambda g: rank(g) < j, a, b)
        out["pairs"].append((j, grid_point(a), grid_point(b), slice_at(a), slice_at(b)))
        if math.frexp(delta)[0] != 0.5:
            g = np.arange(max(a - 64, 1 - (1 << 52)), min(b + 64, 1 << 52) + 1, dtype=np.int64)
            cre = g * GRID
            fd = cre - lo
            with np.errstate(invalid="ignore"):
                exact, estimate = np.trunc(fd / np.float64(delta)), np.trunc(fd * (1.0 / np.float64(delta)))
            for k in np.flatnonzero((exact != estimate) & (cre >= lo)):
                s = slice_at(int(g[k]))
                assert (s if s is not None else n) == min(int(exact[k]), n)
                out["disagree"].append((float(cre[k]), s, int(estimate[k])))
    return out


REPEATING = [  # (step, fixed c or None, sample): candidates -- repeating() keeps what the restatement confirms
    (dict(ship=True), None, (0.0, 0.0)), (dict(degree=3), None, (0.0, 0.0)), (dict(formula=1), None, (0.0, 0.0)),
    (dict(ship=True), None, (-1.0, 0.0)),
    (MANDELBROT, (-1.0, 0.0), (0.0, 0.0)),
    (MANDELBROT, (-2.0, 0.0), (2.0, 0.0)), (MANDELBROT, (-2.0, 0.0), (0.0, 0.0)),
]
REPEATING += [(st, None, (0.0, 0.0)) for st in list(FORMULA_STEPS.values()) + list(POWER_STEPS.values())
              if (st, None, (0.0, 0.0)) not in REPEATING]     # z = c = 0 stays 0 under every step of the table


def repeating(lib, step, c=None, candidates=None):
    """Samples whose orbit under (step, c) never escapes and repeats bit for bit -> [(sample, period, on_the_circle)]:
    each candidate is stepped 121 times with the restatement; it is kept if z_120 is z_60 bit for bit (what the scheduler
    sees at the first boundary where it can: it saves z_60 and compares at 120), and its period is the least p in (1, 2)
    with z_{60+p} == z_60.  on_the_circle: some |z_k|^2 is 4.0 exactly (the strict test keeps it).  -2 itself cannot be
    planted, so c = -2 occurs as a fixed c only."""
    found = []
    for st, cc, sample in (REPEATING if candidates is None else candidates):
        if st != step or cc != c:
            continue
        cr, ci = sample if c is None else c
        r, i = sample
        zs, norms = [], []
        for _ in range(121):
            r, i, m = plot.step(lib, cr, ci, r, i, **step)
            zs.append((r, i))
            norms.append(m)
        bits = [np.array(z).tobytes() for z in zs]                       # bits[k - 1] is z_k
        if max(norms) > 4.0 or bits[119] != bits[59]:
            continue
        period = 1 if bits[60] == bits[59] else 2
        assert bits[59 + period] == bits[59]
        found.append((sample, period, 4.0 in norms))
    return found


def saves_after(chunks):
    """The scheduler's save rule (draw_rounds.h brent_save; tests/phoenix_reference.c saves_after): the chunks done have no
    set bit below their top two -- after 1, 2, 3, 4, 6, 8, 12 ... chunks."""
    top = chunks.bit_length() - 1
    return top < 1 or (chunks & ((1 << (top - 1)) - 1)) == 0


PHOENIX_CYCLES = [  # (p, fixed c or None, sample): candidates -- phoenix_cycles() keeps what the restatement confirms
    ((0.25, 0.0), None, (-0.8125, 0.0)), ((0.25, 0.0), None, (-0.853515625, 0.0)),
    ((-0.5, 0.0), None, (-1.900390625, 0.0)),
    ((-0.5, 0.0), None, (-1.80267333984375, 0.0)),           # z at 180, the state only at 360: across the saves after 3 and 4 chunks
    ((-0.5, 0.0), None, (-1.4501953125, 0.0)),               # z at 180, the state never below 1000 steps
    ((-0.5, 0.0), (-0.8, 0.156), (-1.470703125, 0.078125)),
]


def phoenix_cycles(lib, p, c=None, candidates=None, cap=1000):
    """Samples whose Phoenix orbit under (p, c) never escapes and comes back to a saved z bit for bit -> [(sample, found_z,
    found_state)]: each candidate is stepped at most `cap` times with the restatement's step and compared as
    phoenix_reference.c's one_sample does it, at every k that is a multiple of CHUNK with the point saved last, which is
    then replaced where saves_after(k / CHUNK).  found_z: the first such k at which z alone equals the saved z; found_state:
    the first at which the whole state (z, y) equals the saved state, None if there is none up to cap.  Kept where z is
    found at all and no point up to there (up to found_state, where there is one) escapes."""
    found = []
    for pp, cc, sample in (PHOENIX_CYCLES if candidates is None else candidates):
        if tuple(pp) != tuple(p) or cc != c:
            continue
        cr, ci = sample if c is None else c
        state, saved, found_z, found_state = (float(sample[0]), float(sample[1]), 0.0, 0.0), None, None, None
        for k in range(1, cap + 1):
            *state, m = phoenix.step(lib, cr, ci, p[0], p[1], *state)
            if m > 4.0:
                found_z = None
                break
            if k % CHUNK:
                continue
            bits = [np.float64(v).tobytes() for v in state]
            if saved is not None and bits[:2] == saved[:2]:
                found_z = k if found_z is None else found_z
                if bits == saved:
                    found_state = k
                    break
            if saves_after(k // CHUNK):
                saved = bits
        if found_z is not None:
            found.append((sample, found_z, found_state))
    return found


_CYCLE_SEARCH = {}


def phoenix_cycle_search(p_re, bits=14, cap=1000):
    """Where the candidates of PHOENIX_CYCLES come from, and where a replacement is found should the restatement stop
    confirming one: every real sampled c on the 2^-bits grid in (-2, 2], under a real p that is a power of two.  There z_im
    = y_im = 0, p y is exact and the step is c + RN(z z), then + p y, each one rounding: numpy's doubles do it, all
    samples at once (2^(bits + 2) orbits of `cap` steps: 65 536 of 1000 by default).  -> {(found_z, found_state or None):
    [c_re]} of the samples that never escape and whose z is found before their state, by phoenix_cycles' rule; cached.
    The signs of zeros are not followed here: a candidate counts once phoenix_cycles confirms it on the restatement."""
    key = (float(p_re), bits, cap)
    if key in _CYCLE_SEARCH:
        return _CYCLE_SEARCH[key]
    assert math.frexp(abs(p_re))[0] == 0.5, "p y must be exact"
    c = np.arange(-(2 << bits) + 1, (2 << bits) + 1) / float(1 << bits)
    z, y = c.copy(), np.zeros_like(c)
    alive = np.ones(len(c), dtype=bool)
    saved_z = saved_y = None
    found_z, found_state = np.zeros(len(c), dtype=np.int64), np.zeros(len(c), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(1, cap + 1):
            z, y = (c + z * z) + p_re * y, z
            alive &= ~(z * z > 4.0)
            if k % CHUNK:
                continue
            if saved_z is not None:
                same_z = z == saved_z
                found_z = np.where((found_z == 0) & same_z, k, found_z)
                found_state = np.where((found_state == 0) & same_z & (y == saved_y), k, found_state)
            if saves_after(k // CHUNK):
                saved_z, saved_y = z.copy(), y.copy()
    out = {}
    for j in np.flatnonzero(alive & (found_z > 0) & (found_z != found_state)):
        out.setdefault((int(found_z[j]), int(found_state[j]) or None), []).append(float(c[j]))
    _CYCLE_SEARCH[key] = out
    return out


def cycle_discount(found, max_iter):
    """The steps the early-out saves on a sample found at `found` (None: never): max_iter - found where the comparison is
    made at all, at found < max_iter."""
    return max(max_iter - found, 0) if found is not None else 0


def c_plane_edges(box, w, h):
    """On a canvas with dyadic pixels under plot.C_PLANE, where (u, v) of every orbit point is the sample itself: for
    each axis the coordinate on min, on an inner pixel edge and on max, each with the grid point one step below it ->
    [(axis, name, on, below)]."""
    out = []
    for axis, (lo, hi, n) in enumerate(((box[0], box[1], w), (box[2], box[3], h))):
        inner = lo + (n // 3) * ((hi - lo) / n)
        for name, edge in (("min", lo), ("inner", inner), ("max", hi)):
            out.append((axis, name, edge, grid_point(grid_index(edge) - 1)))
    return out


def projected_orbit(lib, projection, sample, n, c=None, plot_lib=None, **step):
    """(u_k, v_k) of z_1 .. under plot.point, the escaping point included -> (u array, v array, end).  Under a Phoenix step
    `lib` is phoenix_reference's library, and plot_lib is plot_reference's, whose plot.point the render shares."""
    points, end = orbit_of(lib, sample, n, c, **step)
    cr, ci = sample if c is None else c
    uv = np.array([plot.point(plot_lib or lib, projection, r, i, cr, ci) for r, i in points])
    return uv[:, 0], uv[:, 1], end


def hologram_canvases(lib, w, h):
    """pixel_edge_canvases on the plotted coordinates of one planted orbit (end 61) under plot.HOLOGRAM, an irrational
    projection -> (sample, (u, v), {kind: [boxes]})."""
    sample = with_end(lib, 61)
    u, v, end = projected_orbit(lib, plot.HOLOGRAM, sample, 61)
    assert end == 61
    return sample, (u, v), pixel_edge_canvases((u, v), w, h, limit=2)


# ---- the frames render's point queue, modelled (draw_frames.hip, FramesMode::converged and ::drain) -------------------------


def queue_fills(ends, min_iter=1):
    """The wave's LDS queue under one planted sample per lane: ends[lane] is the lane's `end`, None or an end below
    min_iter + 1 for a lane that notes nothing (a filler, a sample that never escapes).  By the scheduler's round rule a lane
    that escapes at step n iterates ceil(n / 12) rounds and replays from the next: in replay round j (0-based) it notes a
    point at hook t (0 .. 11) iff 12 j + t < n.  At every hook count += lanes noting; a count >= 64 drains the newest 64.
    -> (the count before each drain, the remainder drained at `last`)."""
    fills, count, hook = [], 0, {}
    for n in ends:
        if n is None or n - 1 < min_iter:
            continue
        first = -(-n // ROUND)                      # rounds spent iterating
        for p in range(n):
            at = (first + p // ROUND) * ROUND + p % ROUND
            hook[at] = hook.get(at, 0) + 1
    for at in sorted(hook):
        assert hook[at] <= 64
        count += hook[at]
        if count >= 64:
            fills.append(count)
            count -= 64
    return fills, count


# ---- the cases both plotted suites use (tests/test_planted_plot_host.py, tests/test_gpu_planted_plot*.py) -------------------

ENDS = (1, 12, 13, 60, 61, 120, 121)               # a round's last step and the next round's first, likewise for a chunk and two
SHAPES = ("lane0", "lane63", "all64")
WIDE_BOX = (-4.0, 4.0, -3.0, 3.0)                  # 64 x 48 pixels of 1/8: z = 2 (c = -2, z_1 of c = 1) is on it


def lanes(edge, threads=64, shape="lane0", filler=FILLER):
    """One sample per subsequence: the edge sample alone in lane 0 or in lane 63 of the first wave, or in all its 64
    lanes; fillers everywhere else."""
    points = [filler] * threads
    for k in {"lane0": (0,), "lane63": (63,), "all64": range(64)}[shape]:
        points[k] = edge
    return points


def cycled(samples, threads):
    return [samples[k % len(samples)] for k in range(threads)]


def windows_of(end):
    """(max_iter, min_iter) around an orbit's `end`, with what becomes of it: k = end - 1 is the last k accepted under
    max_iter = end; at max_iter = end - 1 the orbit never escapes; min_iter = end - 1 accepts k and min_iter = end does not.
    Wherever it can be min_iter is at least 1, so that the fillers are too fast."""
    return [(end, min(1, end - 1), "recorded"), (end - 1, min(1, max(end - 2, 0)), "never_escaped"),
            (end + 7, end - 1, "recorded"), (end + 7, end, "too_fast")]


def model_counters(ends, max_iter, min_iter):
    """The counters of one launch of one sample per subsequence from the samples' `end`s alone (None: never escapes
    within any max_iter; "rejected": dropped unseen), by the definition: what planted counts must give exactly."""
    c = dict.fromkeys(("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps"), 0)
    for end in ends:
        c["samples"] += 1
        if end == "rejected":
            c["rejected"] += 1
        elif end is None or end > max_iter:
            c["never_escaped"] += 1
            c["iterate_steps"] += max(max_iter, 0)
        else:
            c["iterate_steps"] += end
            if end - 1 < min_iter:
                c["too_fast"] += 1
            else:
                c["recorded"] += 1
                c["replay_steps"] += end
    return c


# The depth windows along `cr`.  The first two are tests/test_gpu_depth.py's (test_the_slice_arithmetic_is_the_row_arithmetic):
# their deltas, 1/2 and 1/4, are both powers of two, so both take the reciprocal; the third (test_gpu_depth.py's
# mandelbrot_cr_inner) has delta 0.18 and takes the division, and at c_re = -0.54 the two paths would differ.
SLICE_WINDOWS = {"reciprocal_5": (-2.0, 0.5, 5), "reciprocal_8": (-1.0, 1.0, 8), "division_5": (-0.9, 0.0, 5),
                 "one": (-1.0, 1.0, 1), "most": (-1.0, 1.0, 256)}
C_BOX = (0.5, 0.75, 0.25, 0.4375)  # 64 x 48 pixels of 2^-8, right of the cardioid: every c on it escapes within a few steps


def c_plane_sample(axis, coordinate):
    """The sample of C_BOX with the given coordinate on one axis and an inner one, off every pixel edge, on the other."""
    return (coordinate, 0.25 + 0.09375 + 5 * GRID) if axis == 0 else (0.5 + 0.109375 + 3 * GRID, coordinate)


def consults_the_map(max_iter, min_iter):
    """Whether the projected product kernel of the Mandelbrot step on a sampled c is given the interior map: where the
    normal path has a LONG stage (capi.hip plot_args; draw_wave.hip plan_stages)."""
    mid = 16 if min_iter <= HEAD_STEPS + MID_MIN else MID_MIN + (min_iter - HEAD_STEPS - MID_MIN) % CHUNK
    return max_iter > HEAD_STEPS + mid


def accepted_beside(lib, c_re, lo=2, hi=400):
    """An imaginary part for the given real parts (a pair of grid neighbours) with which each is a sample the Mandelbrot
    render accepts under min_iter = 1: not rejected, lo <= end <= hi -> (c_im, [ends])."""
    for c_im in (1.125, 0.875, 0.75, 0.6875, 0.625, 0.5, 0.40625, 0.3125, 0.125, 0.0):
        ends = [end_of(lib, (x, c_im), hi + 1) for x in c_re]
        if all(e is not None and lo <= e <= hi for e in ends) and not any(rejected(x, c_im) for x in c_re):
            return c_im, ends
    raise ValueError("no accepted sample with real part %r" % (c_re,))


# ---- the cases both Phoenix suites use (tests/test_planted_phoenix_host.py, tests/test_gpu_planted_phoenix.py) ----------------
#
# On phoenix_reference.load's library.  A setting is (p, fixed c or None).

PHOENIX_SETTINGS = {"sampled": ((-0.5, 0.0), None), "fixed": ((-0.5, 0.0), PHOENIX_C), "sampled_complex": ((0.3, -0.4), None)}
PHOENIX_BOUNDS = {"p_max": ((2.0, 2.0), None), "p_min": ((-2.0, -2.0), None)}   # the bounds the ABI accepts: fewer ends exist
BOUND_ENDS = (1, 12, 13)                           # what the rays must have there at the least

# On the escape circle, p = (-1/2, 0).  Sampled c = 1: z_1 = 1 + 1 = 2 and |z_1|^2 is 4.0 exactly, z_2 = 4 + 1 - 1/2 = 4.5:
# `end` is 2, and a test with >= would make it 1.  Fixed c = -2 from z_0 = 2: z_1 = 2, z_2 = 4 - 2 - 1 = 1, z_3 = 1 - 2 - 1 =
# -2: |z_1|^2 = |z_3|^2 = 4.0 exactly, and no later point escapes.  -> (p, c, sample, the steps on the circle, end)
PHOENIX_CIRCLE = {"sampled": ((-0.5, 0.0), None, (1.0, 0.0), (1,), 2), "fixed": ((-0.5, 0.0), (-2.0, 0.0), (2.0, 0.0), (1, 3), None)}

# The replay plant, by hand: p = (-1/2, 1/4), c = z_0 = (3/4, 1/4), every operation exact.
#   z_1 = (9/16 - 1/16 + 3/4, 2 * 3/4 * 1/4 + 1/4) = (5/4, 5/8), |z_1|^2 = 125/64 < 4, and y_1 = z_0;
#   z_2 = (25/16 - 25/64 + 3/4, 2 * 5/4 * 5/8 + 1/4) + p y_1 = (123/64, 29/16) + (-3/8 - 1/16, -1/8 + 3/16) = (95/64, 15/8),
#   |z_2|^2 > 4: `end` is 2, and both points are on WIDE_BOX.  ITERATE ends with y = z_1; a REPLAY that began with it in the
#   place of 0 would make z_1 = (5/4, 5/8) + p z_1 = (5/4 - 5/8 - 5/32, 5/8 - 5/16 + 5/16) = (15/32, 5/8): another pixel.
PHOENIX_REPLAY = dict(p=(-0.5, 0.25), sample=(0.75, 0.25), end=2, points=[(1.25, 0.625), (1.484375, 1.875)],
                      wrong_first=(0.46875, 0.625))

# Negative zeros: a p and a fixed c whose zero parts carry the sign, from z_0 = 0.  Under p = (-0, -0) the orbit of c = (-1, -0)
# is 0 -> -1 -> 0 ... in value, and the sign of its zero imaginary part has period 4; under p = (-1/2, -0) it passes a -0
# once and settles.  -> (p, c, sample)
PHOENIX_ZEROS = {"p_half": ((-0.5, -0.0), (-1.0, -0.0), (0.0, 0.0)), "p_zero": ((-0.0, -0.0), (-1.0, -0.0), (0.0, 0.0))}
ZEROS_MAX_ITERS = (120, 121, 181, 300)


def cycle_max_iters(found_z, found_state):
    """The max_iter values at which a cycle plant is run: either side of the step at which z alone is found, either side
    of the one at which the state is, and a chunk later (where the state is never found: a chunk later and 1000)."""
    late = (found_state, found_state + 1, found_state + CHUNK) if found_state is not None else (found_z + CHUNK, 1000)
    return (found_z, found_z + 1) + late


def last_save_before(k):
    """The step of the last save made before the comparison at step k (a multiple of CHUNK)."""
    return max(n * CHUNK for n in range(1, k // CHUNK) if saves_after(n))


# ---- six planted outputs: a sample of the cell-list source (draw_cells.h, next_sample<true>; tests/cells_reference.h) ---------
#
# A cell-sourced sample is six outputs: a, b pick the entry j = high half of (a << 32 | b) * n_cells; (x1, x2) and (y1, y2)
# are the offset draws v = o | (o' >> 11) << 32 of either axis, and the coordinate is ONE rounded addition of the cell's
# corner -2 + col 2^-L and the offset (v + 1) 2^-(53 + L), both exact.  Everything here is integers and Fractions: it shares
# no arithmetic with the kernels nor with tests/cells_reference.h.

C_PLANE = plot.C_PLANE                             # --plane cr,ci: every plotted point of an orbit is its c
V_MAX = (1 << 53) - 1                              # the largest offset draw: the next cell's corner, 2 in the last column
SEARCH_BATCH = 1 << 20
_SIX = {}                                          # planted six-output states, by (outputs, free bits, variant)


def _f_np(x):
    t = x ^ (x >> np.uint32(2))
    return t ^ (t << np.uint32(1))


def _g_np(v):
    return v ^ (v << np.uint32(4))


def six_outputs(state):
    """The first six outputs of a state (which is left as it was)."""
    st = oracle.Xorwow(int(state["d"]), (C.c_uint32 * 5)(*[int(v) for v in state["x"]]))
    return [int(oracle.lib.orc_xorwow_next(C.byref(st))) for _ in range(6)]


def plant_outputs(o, free_low_bits_of_o6=11, start=0):
    """An oracle state whose first five outputs are o[0] .. o[4] and whose sixth agrees with o[5] in all but its low
    `free_low_bits_of_o6` bits.  d is searched: from `start` on, batch by batch through all 2^32 values if need be, and the
    first d found whose sixth output fits is taken -- exactly, never nearly; no d at all (chance e^-2048 at 11 free bits) raises."""
    o = [int(v) & M32 for v in o]
    free = int(free_low_bits_of_o6)
    assert len(o) == 6 and 0 <= free < 32
    o1, o5, want = np.uint32(o[0]), np.uint32(o[4]), np.uint32(o[5] >> free)
    k1, k5, k6 = np.uint32(K), np.uint32(5 * K & M32), np.uint32(6 * K & M32)
    step = np.arange(SEARCH_BATCH, dtype=np.uint64)
    for batch in range((1 << 32) // SEARCH_BATCH):
        # candidate number i is start + i * (an odd constant): every d once, and neighbours differ in their high bits (the
        # sixth output's upper bits depend on d's upper bits alone, so consecutive d would repeat one miss 2^7 times)
        i = step + np.uint64(batch * SEARCH_BATCH)
        d = ((i * np.uint64(0x9E3779B1) + np.uint64(int(start) & M32)) & np.uint64(M32)).astype(np.uint32)
        sixth = d + k6 + (_g_np(o5 - d - k5) ^ _f_np(o1 - d - k1))           # u32 arrays: every operation mod 2^32
        hits = np.flatnonzero((sixth >> np.uint32(free)) == want)
        if len(hits):
            break
    else:
        raise ValueError("no generator state has the outputs %r" % (o,))
    d = int(d[hits[0]])
    v = [None] + [(o[n - 1] - d - n * K) & M32 for n in range(1, 6)]
    x4 = _f_inverse(v[5] ^ _g(v[4]))
    x = [_f_inverse(v[1] ^ _g(x4))] + [_f_inverse(v[n] ^ _g(v[n - 1])) for n in range(2, 5)] + [x4]
    state = np.zeros((), dtype=oracle.STATE_DTYPE)
    state["d"] = d
    state["x"] = x
    got = six_outputs(state)
    assert got[:5] == o[:5] and got[5] >> free == o[5] >> free, (o, got)
    return state


def cell_outputs(ab, vx, vy, low=0):
    """The six outputs of the entry draw ab (64 bits) and the offset draws vx, vy (53 bits each); the 11 low bits of the
    fourth output are `low`, those of the sixth are left to plant_outputs."""
    assert 0 <= ab < 1 << 64 and 0 <= vx <= V_MAX and 0 <= vy <= V_MAX
    return (ab >> 32, ab & M32, vx & M32, ((vx >> 32) << 11) | (low & 0x7FF), vy & M32, (vy >> 32) << 11)


def plant_cell_states(draws, variants=2):
    """One state per (ab, vx, vy), subsequence by subsequence.  Subsequence k takes variant k % variants of its draws -- another
    d, other free bits, so another continuation -- and every (draws, variant) is searched once per process."""
    out = np.zeros(len(draws), dtype=oracle.STATE_DTYPE)
    for k, (ab, vx, vy) in enumerate(draws):
        key = (ab, vx, vy, k % variants)
        if key not in _SIX:
            mix = ((k % variants + 1) * 2654435761 + (ab ^ vx ^ vy) * 40503) & M32
            _SIX[key] = plant_outputs(cell_outputs(ab, vx, vy, low=mix >> 7), start=mix)
        out[k] = _SIX[key]
    return out


def exact_entry(ab, n_cells):
    return (ab * n_cells) >> 64


def cell_corner(level, cell):
    """(re, im) of the cell's corner, exact."""
    n = 4 << level
    return Fraction(cell % n, 1 << level) - 2, Fraction(cell // n, 1 << level) - 2


def cell_at(level, re, im):
    """The cell that holds the point (2 is in the last one)."""
    n = 4 << level
    col, row = (min(int((Fraction(x) + 2) * (1 << level)), n - 1) for x in (re, im))
    return row * n + col


def exact_point(level, cell, vx, vy):
    """The sample of the cell at the offset draws, by the definition: the exact corner plus the exact offset as Fractions,
    rounded once by float()."""
    return tuple(float(corner + Fraction(v + 1, 1 << (53 + level))) for corner, v in zip(cell_corner(level, cell), (vx, vy)))


def two_roundings(level, cell, vx, vy):
    """What -2 + (col side + offset) gives: the sum a kernel must NOT compute."""
    n, side = 4 << level, 2.0 ** -level
    return tuple(-2.0 + (float(k) * side + float(v + 1) * 2.0 ** -(53 + level)) for k, v in ((cell % n, vx), (cell // n, vy)))


def exact_sample(level, cells, ab, vx, vy):
    """(j, re, im) of six draws on a list, by exact_entry and exact_point."""
    j = exact_entry(ab, len(cells))
    return (j,) + exact_point(level, int(cells[j]), vx, vy)


def draw_range(level, cell, x):
    """The least and the largest offset draw v with which the coordinate is the double x exactly (corner + offset rounds to
    x), or None if no draw gives x.  Per axis: `cell` is the column or row number."""
    corner = Fraction(cell, 1 << level) - 2

    def at(v):
        return float(corner + Fraction(v + 1, 1 << (53 + level)))

    def first(pred):                                  # the least v in [0, V_MAX + 1] with pred(at(v)); at is monotone
        lo, hi = -1, V_MAX + 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if pred(at(mid)) else (mid, hi)
        return hi

    least, above = first(lambda y: y >= x), first(lambda y: y > x)
    return (least, above - 1) if above > least else None


def draw_of(level, cell, x):
    """The least draw of draw_range."""
    found = draw_range(level, cell, x)
    return None if found is None else found[0]


def draws_for(level, cells, entry, re, im):
    """(ab, vx, vy) that give exactly (re, im) from list entry `entry`: ab in the middle of the entry's range."""
    n, cell = 4 << level, int(cells[entry])
    vx, vy = draw_of(level, cell % n, re), draw_of(level, cell // n, im)
    assert vx is not None and vy is not None, (level, cell, re, im)
    ab = ((2 * entry + 1) << 64) // (2 * len(cells))
    assert exact_sample(level, cells, ab, vx, vy) == (entry, re, im)
    return ab, vx, vy


def entry_edges(n_cells):
    """The entry draws on the edges of j = high half of ab n_cells -> [(ab, j)]: 0 and 2^64 - 1, and for k = 1 and
    n_cells - 1 the pair ceil(k 2^64 / n) - 1, ceil(k 2^64 / n)."""
    out = [(0, 0), ((1 << 64) - 1, n_cells - 1)]
    for k in sorted({1, n_cells - 1} - {0, n_cells}):
        edge = -((-k << 64) // n_cells)
        out += [(edge - 1, k - 1), (edge, k)]
    assert all(exact_entry(ab, n_cells) == j for ab, j in out)
    return out


# four cells outside the set, far apart, whose samples escape after a step or more and whose z_1 is on WIDE_BOX
BEACONS = [(-1.5, 0.5), (0.5, -1.0), (-0.5, 1.0), (1.0, 0.75)]
LIST_SIZES = {"1": (4, 1), "2": (4, 2), "3": (4, 3), "7": (10, 7), "prime": (10, 999983), "grid": (10, 1 << 24)}


def spread_list(level, n_cells):
    """A list whose neighbouring entries are far-apart cells: entry j is cell j M + n^2 / 3 mod n^2 for an odd M near
    n^2 / phi (neighbours lie 0.38 of the grid apart, rows and all), and entries 0, 1, n - 2 and n - 1, the ones the edges
    of the entry draw select, are the BEACONS."""
    total = (4 << level) ** 2
    m = int(total * 0.6180339887) | 1
    cells = ((np.arange(n_cells, dtype=np.uint64) * np.uint64(m) + np.uint64(total // 3)) % np.uint64(total)).astype(np.uint32)
    for j, (re, im) in zip((0, 1, n_cells - 2, n_cells - 1), BEACONS):
        if 0 <= j < n_cells:
            cells[j] = cell_at(level, re, im)
    return cells


def filler_draws(n_cells):
    """The six draws of FILLER from a list whose LAST entry is the grid's last cell: c = (2, 2) exactly."""
    return ((1 << 64) - 1, V_MAX, V_MAX)


def last_cell(level):
    return (4 << level) ** 2 - 1


def ulp_canvas(re, im, w=64, h=48):
    """A canvas whose pixels are one ulp of re wide and one ulp of im high, with (re, im) in pixel (w / 2, h / 2): under
    C_PLANE the histogram reads a sample to the bit.  Every operation of the binning is exact on it."""
    ur, ui = math.ulp(re), math.ulp(im)
    return (re - (w // 2) * ur, re + (w // 2) * ur, im - (h // 2) * ui, im + (h // 2) * ui)


CORNER_CLASSES = {                                 # name -> the cell's column corner as a function of the level
    "[-2,-1)": lambda level: Fraction(-3, 2),
    "[-1,-1/2)": lambda level: Fraction(-3, 4),
    "[1/2,1)": lambda level: Fraction(3, 4),
    "-2^-L": lambda level: Fraction(-1, 1 << level),
    "0": lambda level: Fraction(0),
}


def tie_draws(level, corner):
    """Offset draws of the cell with the given corner coordinate whose exact sum corner + offset is a tie of the result's
    format, and one unit of the offset either side: [(v, tie parity or None, what)] -- for the two corners near zero,
    where every sum is exact, the same draws (no tie there: what = "exact")."""
    unit = Fraction(1, 1 << (53 + level))
    ulp = Fraction(math.ulp(float(corner + Fraction(1, 2 << level))))        # of the cell's middle: one binade per cell
    r = int(ulp / unit)
    if r < 2:                                                                 # beside zero: the sum is exact whatever the draw
        r = 1 << level
    else:
        assert (corner / ulp).denominator == 1
    out = []
    for t in ((1 << 52) // r + 12345, (1 << 52) // r + 12346):               # both parities of the kept bit, mid-cell
        m = t * r + r // 2
        exact = corner + m * unit
        tie = (exact / ulp - Fraction(1, 2)).denominator == 1
        for dm, what in ((-1, "below"), (0, "tie" if tie else "exact"), (1, "above")):
            out.append((m + dm - 1, t & 1 if tie else None, what))
    return out


def interior_edges(limit=3, level=10):
    """From the shipped interior map: column edges E in (-1, 0) with an unmarked cell on the left and a marked one on the
    right, in rows where neither (E - ulp, im) nor (E, im) is in the cardioid or the bulb -> [(E, im, map level)], im the
    middle of the map's row."""
    import gzip
    import struct

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = gzip.open(os.path.join(root, "cudabrot_amd", "interior_map.bin.gz"), "rb").read()
    _, map_level, cols, rows = struct.unpack("<4I", raw[:16])
    bits = np.unpackbits(np.frombuffer(raw, dtype=np.uint8, offset=16), bitorder="little")[:rows * cols].reshape(rows, cols)
    side = 2.0 ** -map_level
    out = []
    for row in range(rows // 7, rows, rows // 5):                             # a few rows, apart
        for col in np.flatnonzero(bits[row, 1:] & ~bits[row, :-1] & 1) + 1:
            e, im = -2.0 + int(col) * side, (row + 0.5) * side
            below = math.nextafter(e, -math.inf)
            if -1.0 < e < 0.0 and not rejected(below, im) and not rejected(e, im):
                out.append((e, im, map_level))
                break
        if len(out) == limit:
            break
    return out


def map_columns(c_re, map_level):
    """(the column of the cell that holds c_re, the column the rounded sum c_re + 2 gives)."""
    return math.floor(Fraction(c_re) * (1 << map_level)) + (2 << map_level), int(math.ldexp(c_re + 2.0, map_level))


def _adjacent(pred, inside, outside):
    """Bisects the doubles between inside (pred holds) and outside (it does not) -> adjacent doubles (in, out)."""
    assert pred(inside) and not pred(outside)
    while math.nextafter(inside, outside) != outside:
        mid = inside + (outside - inside) / 2
        if mid in (inside, outside):
            mid = math.nextafter(inside, outside)
        if pred(mid):
            inside = mid
        else:
            outside = mid
    return inside, outside


def shape_edges_off_the_grid():
    """Pairs of ADJACENT doubles (rejected, not rejected) in c_re across the edge of the cardioid and of the bulb, at real
    parts whose ulp is finer than the 2^-51 grid of the four-draw samples, both members off that grid: only a cell-sourced
    sample can be there.  -> [(shape, (re in, im), (re out, im))]"""
    rays = [("cardioid", 0.3, 0.0, 0.45), ("cardioid", -0.3, 0.0, 0.45), ("cardioid", 0.6, -0.3, -0.7),
            ("cardioid", 0.0625 + 2.0 ** -30, 0.0, 0.45), ("bulb", 0.1, -0.9, -0.7), ("bulb", -0.2, -0.9, -0.7),
            ("bulb", 0.2, -0.95, -0.7), ("bulb", 0.125 + 2.0 ** -33, -0.9, -0.7)]
    out = []
    for shape, im, inside, outside in rays:
        pred = oracle.lib.orc_in_main_cardioid if shape == "cardioid" else oracle.lib.orc_in_order2_bulb
        a, b = _adjacent(lambda x: bool(pred(x, im)), inside, outside)
        off = [math.ldexp(x, 51) != int(math.ldexp(x, 51)) for x in (a, b)]
        if all(off) and rejected(a, im) and not rejected(b, im):
            out.append((shape, (a, im), (b, im)))
    return out


# ---- the mask sink: uniform-source samples on the edges of mark_cell (draw_cells.h) ------------------------------------------

GUARD_WORDS = 64


def mask_bit(level, re, im):
    """(word, bit) of the mask that the sample's cell is."""
    index = cell_at(level, re, im)
    return index >> 5, index & 31


def cell_edge_samples(level):
    """Samples on a cell edge and their 2^-51 neighbours below it, chosen by the bit they mark: bit 0 and bit 31, the
    first and the last word; and c = 2 on re, on im and on both -> [(name, (re, im))].  -2 cannot be planted: a sample of the
    normal stream is never below -2 + 2^-51."""
    n, s = 4 << level, 2.0 ** -level
    half = s / 2
    low, high = -2.0 + half, 2.0 - half              # the middles of the first and the last column (row)
    edge = lambda k: -2.0 + k * s                    # noqa: E731
    below = lambda x: grid_point(grid_index(x) - 1)  # noqa: E731
    out = []
    for name, re, im in (("row 0, column 32", edge(32), low), ("last row, column n - 32", edge(n - 32), high),
                         ("last row, last column", edge(n - 1), high)):
        out += [(name + ": on the edge", (re, im)), (name + ": below it", (below(re), im))]
    for name, re, im in (("column 0, row 1", low, edge(1)), ("column 31, row 1", edge(31) + half, edge(1)),
                         ("last column, last row", high, edge(n - 1))):
        out += [(name + ": on the edge", (re, im)), (name + ": below it", (re, below(im)))]
    out += [("re = 2", (2.0, 0.5)), ("im = 2", (0.5, 2.0)), ("both = 2", (2.0, 2.0)),
            ("the first cell", (grid_point(1 - (1 << 52)), grid_point(1 - (1 << 52))))]
    return out


def box_around(point, half=0.25):
    """A 64 x 48 canvas of dyadic extent with the point well inside."""
    r, i = (math.floor(x * 8) / 8 for x in point)
    return (r - half, r + half, i - half, i + half)


def box_from(point, extent=0.5):
    """A canvas whose LOWER edges are the point's coordinates exactly: the point is in pixel (0, 0), and whatever lies below
    it on either axis is off the canvas."""
    return (point[0], point[0] + extent, point[1] - extent / 2, point[1] + extent / 2)


def filler_marks(box):
    """Whether z_1 of FILLER, (2, 10), its only replayed point under min_iter 0, is on the canvas."""
    return box[0] <= 2.0 < box[1] and box[2] <= 10.0 < box[3]


NOWHERE = (10.0, 10.5, 10.0, 10.5)                 # |z| <= 2^2 + |c| < 7 for every plotted point: no orbit comes here


# ---- the cases both cell suites use (tests/test_planted_cells_host.py, tests/test_gpu_planted_cells.py) -----------------------
#
# A cell case is (level, list, [(ab, vx, vy)] of the planted sample, the sample by exact_sample).  The lists of the cases that
# idle their other lanes end with the grid's last cell, from which filler_draws gives FILLER itself.

MID = (1 << 52) - 1                                # the offset draw of a cell's middle
CELL_MAX_ITER = 121
_LISTS = {}


def sized_list(name):
    if name not in _LISTS:
        _LISTS[name] = spread_list(*LIST_SIZES[name])
    return LIST_SIZES[name][0], _LISTS[name]


def entry_plants(name):
    """The entry draws of entry_edges on the list of that name, each with the cell's middle as its offset ->
    (level, list, [((ab, vx, vy), j)])."""
    level, cells = sized_list(name)
    return level, cells, [((ab, MID, MID), j) for ab, j in entry_edges(len(cells))]


def listed(level, *points):
    """A list of the cells that hold the points, in their order, and then the grid's last cell."""
    return np.array([cell_at(level, *p) for p in points] + [last_cell(level)], dtype=np.uint32)


def offset_plants(level):
    """Offset extremes -> [(name, list, draws, neighbour draws or None)]: v = 0 and v = 2^53 - 1 on either axis of an inner
    cell whose corner on that axis is 0 (the cells of (0, 5/4) and of (1, 0), outside the set) -- beside zero every draw
    gives another double, so the neighbour is v + 1 or v - 1 --, and v = 2^53 - 1 in the last column, the last row and the
    last cell: c = 2 exactly, where the neighbour is the largest draw that still gives the double below 2."""
    n, out = 4 << level, []
    inner = listed(level, (0.0, 1.25), (1.0, 0.0))
    first, second = 1 << 61, 1 << 63                                           # entry draws of the list's entries 0 and 1
    for name, ab, vx, vy, wx, wy in (("re: v = 0", first, 0, MID, 1, MID), ("re: v = max", first, V_MAX, MID, V_MAX - 1, MID),
                                     ("im: v = 0", second, MID, 0, MID, 1), ("im: v = max", second, MID, V_MAX, MID, V_MAX - 1)):
        out.append(("inner, " + name, inner, (ab, vx, vy), (ab, wx, wy)))
    under = draw_range(level, n - 1, math.nextafter(2.0, 0.0))[1]
    assert draw_range(level, n - 1, 2.0) == (under + 1, V_MAX)                 # every draw above it gives 2
    edge = listed(level, (2.0, 0.5), (0.5, 2.0))
    third = (1 << 64) // 3
    out.append(("last column: re = 2", edge, (third // 2, V_MAX, MID), (third // 2, under, MID)))
    out.append(("last row: im = 2", edge, (third + third // 2, MID, V_MAX), (third + third // 2, MID, under)))
    out.append(("last cell: both = 2", edge, filler_draws(3), None))
    return out


def tie_plants(level, axis):
    """[(class, list, draws, tie parity, what)] of tie_draws on the given axis, in a cell outside the set: beside the row
    of corner 5/4 (axis 0) or the column of corner 1 (axis 1)."""
    out = []
    for name, corner in CORNER_CLASSES.items():
        x = float(corner(level))
        cells = listed(level, (x, 1.25) if axis == 0 else (1.0, x))
        for v, parity, what in tie_draws(level, corner(level)):
            out.append((name, cells, (1 << 62, v, MID) if axis == 0 else (1 << 62, MID, v), parity, what))
    return out


def map_plants(level=10):
    """[(E, im, list, draws below E, draws on E, map level)] of interior_edges."""
    out = []
    for e, im, map_level in interior_edges(level=level):
        below = math.nextafter(e, -math.inf)
        cells = listed(level, (below, im), (e, im))
        out.append((e, im, cells, draws_for(level, cells, 0, below, im), draws_for(level, cells, 1, e, im), map_level))
    return out


def shape_plants(level=10):
    """[(shape, list, draws inside, draws outside, (re, im) inside, (re, im) outside)] of shape_edges_off_the_grid."""
    out = []
    for shape, a, b in shape_edges_off_the_grid():
        cells = listed(level, a, b)
        out.append((shape, cells, draws_for(level, cells, 0, *a), draws_for(level, cells, 1, *b), a, b))
    return out


def cell_lanes(draws, threads=64, shape="lane0"):
    return lanes(draws, threads, shape, filler=filler_draws(0))


NECK = lambda e: (-0.75, e * GRID)                 # noqa: E731  a ray away from the cusp's cell: between cardioid and bulb


def z_1(lib, sample, c=None, **step):
    return orbit_of(lib, sample, 1, c, **step)[0][0]


def replay_cases(lib):
    """Where the probe's replay ends -> [(name, sample, end, box, t)]: a sample of the cusp's ray whose orbit escapes at
    `end`, and a canvas whose lower edge is z_t itself, so that z_t is the orbit's first point on it (the ray's orbits climb
    the real axis: every earlier point is below the edge, every later one on the canvas or beyond it); t None: a canvas no
    orbit reaches.  t = 1, t = end (the escaping point), and on an orbit of 121 steps the round's and the chunk's edges."""
    out = []
    for end in ENDS:
        sample = with_end(lib, end)
        points, _ = orbit_of(lib, sample, end)
        for t in sorted({1, end}):
            out.append(("end %d: z_%d" % (end, t), sample, end, box_from(points[t - 1]), t))
    for t in (12, 13, 60, 61, 120):
        out.append(("end 121: z_%d" % t, sample, 121, box_from(points[t - 1]), t))
    out.append(("end 121: no point", sample, 121, NOWHERE, None))
    return out


def unmarking_samples(lib):
    """(window, marker, [samples that must not mark]): under max_iter 120, min_iter 13 a sample of the neck's ray that is
    accepted (end 61), and from the cusp's cell and the shapes one that is too fast (end 13), one that never escapes (end
    121) and two that are rejected -- every one with orbit points on WIDE_BOX."""
    marker = with_end(lib, 61, ray=NECK)
    return (120, 13), marker, [with_end(lib, 13), with_end(lib, 121), (-1.0, 0.0), (0.0, 0.0)]


BOUNDED_MARKS = [  # (name, step, fixed c or None, sample, canvas, t: the first on-canvas point is z_t)
    ("transient", MANDELBROT, (-2.0, 0.0), (0.0, 0.0), box_from((-2.0, 0.0)), 1),       # 0 -> -2 -> 2 -> 2 ...
    ("period", MANDELBROT, (-2.0, 0.0), (0.0, 0.0), box_from((2.0, 0.0)), 2),
    ("the saved point", MANDELBROT, (-2.0, 0.0), (2.0, 0.0), box_from((2.0, 0.0)), 1),  # 2 -> 2 ...: every point is z_60
    ("period 2", MANDELBROT, (-1.0, 0.0), (0.0, 0.0), box_from((0.0, 0.0)), 2),         # 0 -> -1 -> 0 ...
    ("sampled c", dict(ship=True), None, (-1.0, 0.0), box_from((-1.0, 0.0)), 2),        # -1 -> 0 -> -1 ...
]                                                  # and each of them on NOWHERE: no point at all, the cycle found at 120
BOUNDED_MAX_ITER = 180
SQUARE_C = (-2.0, 2.0, -2.0, 2.0)                  # the whole sample plane as a canvas of --plane cr,ci: cells apart, pixels apart
