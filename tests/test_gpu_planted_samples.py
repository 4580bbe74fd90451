"""draw_wide_kernel, draw_wave_kernel and the lock-step kernel on PLANTED samples (tests/planted_samples.py): the first
sample of every subsequence is chosen to the bit -- an orbit that escapes exactly at min_iter, at max_iter, at a LONG
chunk's first or last step; a grid neighbour either side of the cardioid's or the bulb's edge; an orbit with points where
only the replay burst's exact division finds the pixel -- and the generator states that draw them are written over the
launch's own.  Everything else is the product path as shipped: queues, the four LONG slots, the replay bursts, the
stream, the scatter, the carry and the drain.  Random samples reach none of these decisions (tests/
test_planted_samples_host.py shows on the oracle alone that the planted ones are decisive).

Every comparison is bit-exact against oracle.render(..., states=planted): every pixel, every counter of SAME, status 0,
and the generator states after the run.  The shapes are the smallest that still are the product's: 512 subsequences (one
workgroup of the wide kernel), 1 sample per subsequence -- the planted one alone -- and once 50, so that the generator's
own follow it; canvases of at most 333 x 300; a drain launch at the end of every run."""

import numpy as np
import pytest

import planted_samples as P
from device_launches import SQUARE, Launches, assert_same, omp_threads, planar_states

pytestmark = pytest.mark.gpu

WAVE, WIDE, LOCKSTEP = 1, 2, 3
THREADS = 512
W, H = 333, 300

# how a run is made: (the kernel that must take it, the knobs set for it, the variant's name).  "atomics" and "simple" are
# launched without a workspace -- what CUDABROT_AMD_NO_WORKSPACE=1 makes the renderer do; the knob is the renderer's own,
# these launches are the low-level entry point's, and the lock-step kernel takes no workspace at all
MODES = {
    "wide": (WIDE, {}, "CB_KERNEL_DEFAULT"),
    "wave": (WAVE, {"CUDABROT_AMD_NO_WIDE": "1"}, "CB_KERNEL_DEFAULT"),
    "simple": (LOCKSTEP, {}, "CB_KERNEL_SIMPLE"),
    "full": (None, {}, "CB_KERNEL_FULL_ITERATE"),                 # the wide kernel where it takes the window, else wave
    "dense": (WAVE, {"CUDABROT_AMD_DENSE_TESTS": "1"}, "CB_KERNEL_DEFAULT"),       # no sparse LONG stage: not wide's
    "chunked": (WIDE, {"CUDABROT_AMD_TWO_LEVEL": "1"}, "CB_KERNEL_DEFAULT"),
    "atomics": (WAVE, {}, "CB_KERNEL_DEFAULT"),                   # no workspace: every increment a device-scope atomic
    "ship": (WIDE, {}, "CB_KERNEL_DEFAULT"),
}

_references = {}


def reference(oracle, points, w, h, box, max_iter, min_iter, launches, ship=False):
    """oracle.render on the planted states, once per set of arguments whatever kernels are held to it -> (states before,
    (hist, counters), states after as planes); nothing of it is written to afterwards."""
    key = (tuple(points), w, h, tuple(box), max_iter, min_iter, tuple(launches), ship)
    if key not in _references:
        before = P.plant_states(points)
        after = before.copy()
        want = oracle.render(w, h, max_iter, min_iter, len(points), len(launches), box, samples_per_thread=launches[0],
                             states=after, omp_threads=omp_threads(), burning_ship=ship)
        _references[key] = (before, want, planar_states(after))
    return _references[key]


def stream_capacity(cb, dims, nbytes, n_channels=0):
    layout = cb.debug_scatter_layout(dims, THREADS, 4096, nbytes, n_channels)
    return layout.cap * layout.n_waves if layout.enabled else 0


def workspace_bytes(cb, dims, kind, increments, n_channels=0):
    """"roomy": a stream that holds every increment of the run twice over; "small": the smallest the wide kernel still
    takes (64 lanes x 32 steps per stream region), a fraction of the run's increments, so that the bursts add directly.
    n_channels: of a fused launch (tests/test_gpu_planted_channels.py), whose stream words carry a plane's index."""
    planes = max(n_channels, 1)
    if kind == "roomy":
        samples = 50
        while stream_capacity(cb, dims, cb.scatter_workspace_bytes(dims, THREADS, samples, planes),
                              n_channels) < 2 * increments + 65536:
            samples *= 2
        return cb.scatter_workspace_bytes(dims, THREADS, samples, planes)
    nbytes = cb.scatter_workspace_bytes(dims, THREADS, 1, planes)
    while True:
        less = nbytes - 8192
        layout = cb.debug_scatter_layout(dims, THREADS, 4096, less, n_channels) if less > 0 else None
        if layout is None or not layout.enabled or layout.cap < 64 * 32:
            break
        nbytes = less
    assert 4 * stream_capacity(cb, dims, nbytes, n_channels) < increments, "the small stream would hold the run"
    return nbytes


def run(cb, oracle, monkeypatch, key, points, max_iter, min_iter, mode, launches=(1,), *, w=96, h=80, box=SQUARE,
        workspace="roomy", carried=False):
    """One run of `launches` (samples per subsequence, all alike) and a drain on planted states, held to the oracle; key
    names the case in the messages.
    carried: before the drain every sample must be drawn and some not yet decided -- in flight in the carry buffer."""
    assert len(points) == THREADS and len(set(launches)) == 1
    kernel, knobs, variant_name = MODES[mode]
    ship = mode == "ship"
    variant = getattr(cb, variant_name) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    if kernel is None:
        kernel = WIDE if min_iter == P.stage_plan(max_iter, min_iter)[0] else WAVE
    before, want, after = reference(oracle, points, w, h, box, max_iter, min_iter, launches, ship)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    dims = cb.FractalDimensions.make(w, h, *box)
    assert cb.rng_state_bytes(THREADS) == 24 * THREADS
    nbytes = 0 if mode in ("atomics", "simple") else workspace_bytes(cb, dims, workspace, want[1]["increments"])
    if nbytes:      # the stream is chunked by group of tiles where the case says so, and only there
        assert bool(cb.debug_scatter_layout(dims, THREADS, 4096, nbytes).chunked) == (mode == "chunked"), (key, mode)
    seq = Launches(cb, dims, THREADS, workspace=nbytes, carry=True)
    seq.states.copy_(seq.torch.from_numpy(planar_states(before).view(np.uint8)).to(seq.dev))
    it = cb.IterationControl(max_iter, min_iter)
    for n in (*launches, 0):
        if n == 0 and carried:
            so_far = seq.read_counters()
            decided = sum(so_far[k] for k in ("rejected", "never_escaped", "too_fast", "recorded"))
            assert so_far["samples"] == want[1]["samples"] > decided, "%s %s: nothing was carried" % (key, mode)
        assert seq.launch(cb.draw_buddhabrot, n, variant, iterations=it) == kernel, (key, mode)
    got = seq.read()
    for name in knobs:
        monkeypatch.delenv(name)
    keys = [k for k in ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                        "increments") if not (ship and k == "rejected")]
    assert_same(got, want, keys=keys, what="%s %s %r" % (key, mode, launches))
    if ship:
        assert got[1]["rejected"] == 0
    assert np.array_equal(got[3], after), "%s %s: the generator states after the run differ" % (key, mode)
    return got[1]


def both_lengths(cb, oracle, monkeypatch, key, points, max_iter, min_iter, mode, **kw):
    """The planted sample alone, and followed by 49 of the generator's own."""
    alone = run(cb, oracle, monkeypatch, key + "/1", points, max_iter, min_iter, mode, (1,), **kw)
    run(cb, oracle, monkeypatch, key + "/50", points, max_iter, min_iter, mode, (50,), **kw)
    return alone


# ---- window edges ------------------------------------------------------------------------------------------------------


def window_points(max_iter, min_iter, shape="every"):
    samples = P.window_samples(max_iter, min_iter)
    return samples, P.layout([c for _, c in samples], THREADS, shape)


def fates(samples, points, max_iter, min_iter):
    """What the oracle's counters must say of the planted samples alone, from their counts."""
    count_of = {c: n for n, c in samples}
    tally = {"recorded": 0, "too_fast": 0, "never_escaped": 0, "rejected": 0}
    for p in points:
        tally["rejected" if P.rejected(*p) else P.expected_fate(count_of.get(p, 0), max_iter, min_iter)] += 1
    return tally


@pytest.mark.parametrize("mode", ["wide", "wave", "simple", "full", "dense"])
@pytest.mark.parametrize("window", P.WIDE_WINDOWS, ids=lambda w: "%d_%d" % w)
def test_window_edges_of_the_usual_split(cb, oracle, monkeypatch, window, mode):
    """Counts two either side of max_iter (recorded | never escaped) and of min_iter = long_start (too fast | recorded),
    the first LONG chunk's ends, the tail chunk's start: in every lane of a workgroup."""
    max_iter, min_iter = window
    samples, points = window_points(max_iter, min_iter)
    alone = both_lengths(cb, oracle, monkeypatch, "window %r" % (window,), points, max_iter, min_iter, mode)
    tally = fates(samples, points, max_iter, min_iter)
    assert all(alone[k] == v for k, v in tally.items()), (alone, tally)
    assert min(tally["recorded"], tally["too_fast"], tally["never_escaped"]) >= THREADS // 8


@pytest.mark.parametrize("mode", ["wave", "simple", "full", "dense"])
@pytest.mark.parametrize("window", P.PROBE_WINDOWS, ids=lambda w: "%d_%d" % w)
def test_window_edges_with_min_iter_deep_in_the_long_stage(cb, oracle, monkeypatch, window, mode):
    """Both ends of the windows whose min_iter lies hundreds of LONG chunks deep (the wave kernel's probe path): the
    accept / reject decision at min_iter is taken by orbits that reach it, and so is the escape in the last step before
    max_iter, in the tail chunk where there is one."""
    max_iter, min_iter = window
    samples, points = window_points(max_iter, min_iter)
    alone = both_lengths(cb, oracle, monkeypatch, "window %r" % (window,), points, max_iter, min_iter, mode)
    tally = fates(samples, points, max_iter, min_iter)
    assert all(alone[k] == v for k, v in tally.items()), (alone, tally)
    assert min(tally["recorded"], tally["too_fast"], tally["never_escaped"]) >= THREADS // 8


def deep_counts(max_iter, min_iter):
    """The escape counts of the occupancy layouts: two either side of max_iter (the last recorded escapes, and orbits that
    never escape), the steps either side of the tail chunk's start, and one half way through the LONG stage."""
    long_start, tail_start = P.stage_plan(max_iter, min_iter)
    counts = {max_iter + k for k in (-2, -1, 0, 1)} | {tail_start - 1, tail_start + 1, (long_start + max_iter) // 2}
    return sorted(n for n in counts if n <= max_iter + 1)


@pytest.mark.parametrize("mode", ["wide", "wave"])
@pytest.mark.parametrize("shape", ["every", "ends", "b_only"])
def test_occupancy_shapes(cb, oracle, monkeypatch, shape, mode):
    """The same deep orbits -- hundreds of LONG chunks, escapes at max_iter - 1 and in the tail chunk, orbits that never
    escape -- in every lane, in lanes 0 and 63 of one wave only, and in one lane's generator B only, where fewer lanes
    than a replay burst waits for ever replay.  In the two sparse layouts every count gets a run of its own (both rays'
    samples in lanes 0 and 63; the rays in turn in generator B), so each is the only deep work of its wave.  As one launch
    and as two before the drain.  Both product kernels end a launch that has a carry buffer as soon as its samples are
    drawn: the deep orbits are in flight then (asserted before every drain) and leave through the carry and the drain."""
    for max_iter, min_iter in ((1234, 20), (20000, 20)):
        counts = deep_counts(max_iter, min_iter)
        long_start, tail_start = P.stage_plan(max_iter, min_iter)
        assert {max_iter - 2, max_iter - 1, max_iter, max_iter + 1, tail_start - 1} <= set(counts)
        assert min(counts) >= (long_start + max_iter) // 2 and sum(n >= max_iter - 2 for n in counts) == 4
        samples = [(n, P.with_escape_count(n, ray)) for n in counts for ray in ("cusp", "neck")]
        if shape == "every":
            runs = [samples]
        else:       # one count per run: its cusp and its neck sample, the neck one first for every other count
            runs = [samples[2 * k:2 * k + 2][::-1 if k % 2 else 1] for k in range(len(counts))]
        for planted in runs:
            points = P.layout([c for _, c in planted], THREADS, shape)
            deep = [n for n, c in planted if c in points]
            assert len(deep) == {"every": len(samples), "ends": 2, "b_only": 1}[shape]
            assert shape == "every" or min(deep) == max(deep) == planted[0][0]
            key = "occupancy %s %d %r" % (shape, max_iter, deep[:2])
            one = run(cb, oracle, monkeypatch, key + "/1", points, max_iter, min_iter, mode, (1,), carried=True)
            run(cb, oracle, monkeypatch, key + "/1+1", points, max_iter, min_iter, mode, (1, 1), carried=True)
            tally = fates(planted, points, max_iter, min_iter)
            assert all(one[k] == v for k, v in tally.items()), (one, tally)
            assert tally["recorded"] + tally["never_escaped"] == sum(1 for p in points if p not in P.DULL)


# ---- cardioid and bulb -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["wide", "wave", "simple"])
def test_cardioid_and_bulb_pairs(cb, oracle, monkeypatch, mode):
    """Grid neighbours either side of the two shapes' edges (in_main_cardioid2 / in_order2_bulb2 on doubled coordinates,
    and the wide kernel's hand-scheduled form): the inside one of each pair is rejected, the outside one iterated."""
    pairs = P.cardioid_pairs() + P.bulb_pairs()
    flat = [p for pair in pairs for p in pair]
    points = P.layout(flat, THREADS, "every")
    alone = both_lengths(cb, oracle, monkeypatch, "shapes", points, 100, 20, mode)
    inside = sum(1 for p in points if P.rejected(*p))
    assert alone["rejected"] == inside and abs(2 * inside - THREADS) <= 2
    assert alone["samples"] == THREADS == sum(alone[k] for k in ("rejected", "never_escaped", "too_fast", "recorded"))


# ---- pixel edges -------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def edge_cases():
    return P.pixel_edge_cases(W, H)


def edge_layout(samples):
    """The base orbit (1234 points, with the row disagreements) in every other subsequence, the real samples (a few dozen
    points each, with the column disagreements) cycled through the rest."""
    return [samples[0] if k % 2 == 0 else samples[1 + (k // 2) % (len(samples) - 1)] for k in range(THREADS)]


EDGE_RUNS = [("wide", "roomy"), ("chunked", "roomy"), ("wide", "small"), ("wave", "roomy"), ("atomics", "roomy")]


@pytest.mark.parametrize("mode,workspace", EDGE_RUNS, ids=["%s_%s" % r for r in EDGE_RUNS])
def test_pixel_edges_need_the_exact_division(cb, oracle, monkeypatch, edge_cases, mode, workspace):
    """Canvases on which planted orbits have points that trunc(a * RN(1 / delta)) would put into the neighbouring pixel:
    the replay burst's exact-division fallback decides them -- on the blocked one-level stream, the chunked stream, a
    stream too small (the bursts add directly), in the wave kernel, and with direct atomics."""
    base, canvases = edge_cases
    for n, (box, samples) in enumerate(canvases["fallback"]):
        points = edge_layout(samples)
        both_lengths(cb, oracle, monkeypatch, "fallback %d" % n, points, 1234, 20, mode, w=W, h=H, box=box,
                     workspace=workspace)


@pytest.mark.parametrize("mode", ["wide", "chunked", "wave", "atomics"])
def test_points_on_the_canvas_border(cb, oracle, monkeypatch, edge_cases, mode):
    """An orbit point exactly on min_real and one on min_imag (pixel 0, by the exact division: the estimate is 0), the
    same points one ulp below the bounds (not counted), and points exactly on max_real and max_imag."""
    base, canvases = edge_cases
    points = P.layout([base], THREADS, "every")
    for kind in ("on_min", "below_min", "on_max"):
        (box,) = canvases[kind]
        run(cb, oracle, monkeypatch, "border " + kind, points, 1234, 20, mode, (1,), w=W, h=H, box=box)


@pytest.mark.parametrize("mode", ["wide", "chunked", "wave"])
def test_the_same_orbits_on_dyadic_pixels(cb, oracle, monkeypatch, edge_cases, mode):
    """The kPow2 instances of the bursts (one exact fma per coordinate, no division) on the same planted orbits."""
    base, canvases = edge_cases
    points = edge_layout(canvases["fallback"][0][1])
    both_lengths(cb, oracle, monkeypatch, "dyadic", points, 1234, 20, mode, w=256, h=128, box=SQUARE)


def test_pixel_edges_of_the_burning_ship_build(cb, oracle, monkeypatch, edge_cases):
    """The RENDER_BURNING_SHIP instance of the wide kernel's burst on the first canvas, with the real samples (a
    positive real orbit is the same under both steps: tests/test_planted_samples_host.py restates it)."""
    base, canvases = edge_cases
    box, samples = canvases["fallback"][0]
    points = P.layout(samples[1:], THREADS, "every")
    both_lengths(cb, oracle, monkeypatch, "ship", points, 1234, 20, "ship", w=W, h=H, box=box)
