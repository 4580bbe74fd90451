"""cb_draw_buddhabrot_channels, the fused multi-channel render, on PLANTED samples (tests/planted_samples.py, "the cases
both channel suites use"): the first sample of every subsequence escapes exactly at, or next to, a window's min or max, a
LONG chunk's first or last index, the LONG stage's start, the tail chunk's start or the hull's max -- where the kernel
decides whether an orbit is recorded at once or measured first, which planes it goes to, where the sparse chunks'
over-count is taken back and which counter it adds to.  The generator's own samples reach a shallow edge often, a deep one,
a tail chunk's or an orbit in four planes essentially never (tests/test_planted_channels_host.py shows on the oracle alone
that the planted ones do).  Everything else is the product path as shipped: queues, LONG slots, replay bursts with
tagged words, the stream, the scatter over the stacked planes, the carry and the drain.

Every run asserts: plane j bit-equal to oracle.render(window j, states=planted), empty planes included; status 0;
samples, rejected, never_escaped and iterate_steps those of the oracle's run of the hull window; increments the sum of
the planes; the generator states after the run the oracle's; recorded, too_fast and replay_steps equal to fused_model
(the restatement of DESIGN.md 4.6) where the planted sample is alone, and held to the oracle's separate runs where the
generator's own follow it.  512 subsequences, a 96 x 80 canvas, 1 sample per subsequence and once 50."""

import numpy as np
import pytest

import planted_samples as P
from device_launches import SQUARE, Launches, omp_threads, planar_states
from test_gpu_planted_samples import stream_capacity, workspace_bytes

pytestmark = pytest.mark.gpu

THREADS = 512
W, H = 96, 80
SETS = sorted(P.CHANNEL_SETS)

# how a run is made: (the knobs set for it, the variant's name, the workspace).  Every one is draw_wave_kernel's
MODES = {
    "binned": ({}, "CB_KERNEL_DEFAULT", "roomy"),
    "small": ({}, "CB_KERNEL_DEFAULT", "small"),                  # a stream too small: bursts fall to the direct loop mid-run
    "chunked": ({"CUDABROT_AMD_TWO_LEVEL": "1"}, "CB_KERNEL_DEFAULT", "roomy"),
    "atomics": ({}, "CB_KERNEL_DEFAULT", None),                   # no workspace: every increment a device-scope atomic
    "full": ({}, "CB_KERNEL_FULL_ITERATE", "roomy"),
}

_references = {}


def reference(oracle, points, windows, launches, ship=False):
    """The oracle on the planted states, once per set of arguments whatever modes are held to it -> (states before,
    [(hist, counters) per window], counters of the hull window, states after the hull run as planes); nothing of it is
    written to afterwards."""
    key = (tuple(points), tuple(windows), tuple(launches), ship)
    if key not in _references:
        before = P.plant_states(points)

        def render(window):
            states = before.copy()
            out = oracle.render(W, H, window[0], window[1], len(points), len(launches), SQUARE,
                                samples_per_thread=launches[0], states=states, omp_threads=omp_threads(), burning_ship=ship)
            return out, states

        singles = [render(w)[0] for w in windows]
        (_, of_hull), after = render(P.hull(windows))
        _references[key] = (before, singles, of_hull, planar_states(after))
    return _references[key]


def smallest_stream(cb, dims, n_channels):
    """(bytes, capacity) of the smallest stream the kernel still takes."""
    nbytes = workspace_bytes(cb, dims, "small", 1 << 62, n_channels)
    return nbytes, stream_capacity(cb, dims, nbytes, n_channels)


def run(cb, oracle, monkeypatch, key, windows, points, mode, launches=(1,), *, ship=False, carried=False):
    """One run of `launches` (samples per subsequence, all alike) and a drain on planted states, held to the oracle and,
    where the planted sample is alone, to the model; key names the case in the messages.
    carried: before the drain every sample must be drawn and some not yet decided -- in flight in the carry buffer."""
    assert len(points) == THREADS and len(set(launches)) == 1
    what = "%s %s %r" % (key, mode, launches)
    knobs, variant_name, workspace = MODES[mode]
    variant = getattr(cb, variant_name) | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0)
    before, singles, of_hull, after = reference(oracle, points, windows, launches, ship)
    increments = sum(c["increments"] for _, c in singles)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    dims = cb.FractalDimensions.make(W, H, *SQUARE)
    n = len(windows)
    nbytes = workspace_bytes(cb, dims, workspace, increments, n) if workspace else 0
    if nbytes:      # the stream is chunked by group of tiles where the case says so, and only there
        assert bool(cb.debug_scatter_layout(dims, THREADS, 4096, nbytes, n).chunked) == (mode == "chunked"), what
    seq = Launches(cb, dims, THREADS, planes=n, workspace=nbytes, carry=True)
    seq.states.copy_(seq.torch.from_numpy(planar_states(before).view(np.uint8)).to(seq.dev))
    for samples in (*launches, 0):
        if samples == 0 and carried:
            so_far = seq.read_counters()
            decided = sum(so_far[k] for k in ("rejected", "never_escaped", "too_fast", "recorded"))
            assert so_far["samples"] == of_hull["samples"] > decided, "%s: nothing was carried" % what
        assert seq.launch(cb.draw_buddhabrot_channels, samples, variant, windows=windows) == 1, what
    planes, got, _, states = seq.read()
    for name in knobs:
        monkeypatch.delenv(name)

    assert got["status"] == 0, "%s: the kernel reported an internal invariant violation: %r" % (what, got)
    for j, (hist, _) in enumerate(singles):
        if not np.array_equal(planes[j], hist):
            diff = np.argwhere(planes[j] != hist)
            raise AssertionError("%s: plane %d (window %r) differs at %d pixels, first %r: got %d, want %d" % (
                what, j, windows[j], len(diff), tuple(diff[0]), planes[j][tuple(diff[0])], hist[tuple(diff[0])]))
    for k in ("samples", "rejected", "never_escaped", "iterate_steps"):
        assert got[k] == of_hull[k], "%s: counter %s: got %d, the hull window's run has %d" % (what, k, got[k], of_hull[k])
    assert got["increments"] == int(planes.sum()) == increments, what
    assert np.array_equal(states, after), "%s: the generator states after the run differ" % what

    # recorded, too_fast, replay_steps: by the oracle's separate runs ...
    accepted = of_hull["samples"] - of_hull["rejected"] - of_hull["never_escaped"]
    assert got["recorded"] + got["too_fast"] == accepted, (what, got, accepted)
    assert got["recorded"] == P.recorded_by_windows(windows, [c["recorded"] for _, c in singles], of_hull["recorded"]), what
    low = sum(c["replay_steps"] for _, c in singles)        # one pass per plane; at most a measuring pass per accepted orbit
    assert low <= got["replay_steps"] <= low + of_hull["replay_steps"], (what, low, got["replay_steps"], of_hull["replay_steps"])
    if tuple(launches) == (1,):                             # ... and, the planted sample alone, exactly by the model
        model = P.fused_model(windows, P.counts_of(points, P.hull(windows)[0] + 2, ship))
        for k in ("rejected", "never_escaped", "too_fast", "recorded", "replay_steps"):
            assert got[k] == model[k], "%s: counter %s: got %d, the model has %d" % (what, k, got[k], model[k])
    return got


def both_lengths(cb, oracle, monkeypatch, key, windows, points, mode, **kw):
    """The planted sample alone, and followed by 49 of the generator's own."""
    alone = run(cb, oracle, monkeypatch, key + "/1", windows, points, mode, (1,), **kw)
    run(cb, oracle, monkeypatch, key + "/50", windows, points, mode, (50,), **kw)
    return alone


# ---- every set in every mode ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", [m for m in MODES if m != "small"])
@pytest.mark.parametrize("name", SETS)
def test_window_edges_of_every_set(cb, oracle, monkeypatch, name, mode):
    """Counts either side of every window edge, chunk end and stage start of the set, in every lane of a workgroup."""
    windows = P.CHANNEL_SETS[name]
    _, points = P.channel_layout(windows, THREADS)
    both_lengths(cb, oracle, monkeypatch, name, windows, points, mode)


@pytest.mark.parametrize("name", SETS)
def test_window_edges_on_a_stream_too_small(cb, oracle, monkeypatch, name):
    """The same on the smallest stream the kernel takes, which must hold less than a quarter of the run's increments (the
    oracle's): the bursts fill it and the direct loop takes over mid-run.  A shallow set's launch of 1 or 50 samples per
    subsequence has too few increments for that; the first two lengths of 1, 50, 400, 3200 that have enough are run."""
    windows = P.CHANNEL_SETS[name]
    _, points = P.channel_layout(windows, THREADS)
    dims = cb.FractalDimensions.make(W, H, *SQUARE)
    _, capacity = smallest_stream(cb, dims, len(windows))
    ran = 0
    for samples in (1, 50, 400, 3200):
        _, singles, _, _ = reference(oracle, points, windows, (samples,))
        if 4 * capacity < sum(c["increments"] for _, c in singles):
            run(cb, oracle, monkeypatch, name, windows, points, "small", (samples,))
            ran += 1
        if ran == 2:
            break
    assert ran == 2, (name, capacity)


# ---- the other step, the other orders -------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["recipe_small", "nested_four"])
def test_the_burning_ship_build(cb, oracle, monkeypatch, name):
    """launch_draw_wave_ship's multi path against the oracle's RENDER_BURNING_SHIP build: the cusp ray's samples have the
    same orbits under both steps (positive and real), the neck ray's other ones -- the model takes the oracle's count of
    each under that step."""
    windows = P.CHANNEL_SETS[name]
    _, points = P.channel_layout(windows, THREADS)
    alone = both_lengths(cb, oracle, monkeypatch, name + " ship", windows, points, "binned", ship=True)
    assert alone["rejected"] == 0 and alone["recorded"] >= THREADS // 8


def test_plane_j_follows_window_j_in_every_order(cb, oracle, monkeypatch):
    """recipe_small with its windows in every cyclic order: the lowest set bit is the first plane recorded into, whatever
    window it stands for."""
    windows = P.CHANNEL_SETS["recipe_small"]
    _, points = P.channel_layout(windows, THREADS)
    counters = []
    for k in range(len(windows)):
        order = windows[k:] + windows[:k]
        counters.append(both_lengths(cb, oracle, monkeypatch, "order %d" % k, order, points, "binned"))
    same = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps", "increments")
    assert all(c[k] == counters[0][k] for c in counters for k in same)


# ---- occupancy -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["every", "ends", "b_only"])
@pytest.mark.parametrize("name", ["nested_four", "edges_one_past_a_start"])
def test_occupancy_shapes(cb, oracle, monkeypatch, name, shape):
    """One orbit of every kind the set has -- its planes, direct or measured -- and one that never escapes: in every lane,
    in lanes 0 and 63 of one wave only, and in one subsequence only, where fewer lanes than a replay burst waits for ever
    replay, so an orbit waits in its lane between its channel passes.  In the two sparse layouts every count gets a run
    of its own.  As one launch and as two before the drain: a launch with a carry buffer ends as soon as its samples are
    drawn, the planted orbits are in flight then (asserted before every drain) and leave through the carry and the
    drain.  With every lane planted, two launches of 50 samples as well: there the replay runs between the draws, and
    orbits between two of their passes cross the launch with their tag and their flags in the carry."""
    windows = P.CHANNEL_SETS[name]
    counts = P.occupancy_counts(windows)
    samples = [(n, P.with_escape_count(n, ray)) for n in counts for ray in ("cusp", "neck")]
    if shape == "every":
        runs = [samples]
    else:           # one count per run: its cusp and its neck sample, the neck one first for every other count
        runs = [samples[2 * k:2 * k + 2][::-1 if k % 2 else 1] for k in range(len(counts))]
    for planted in runs:
        points = P.layout([c for _, c in planted], THREADS, shape)
        deep = [n for n, c in planted if c in points]
        assert len(deep) == {"every": len(samples), "ends": 2, "b_only": 1}[shape]
        key = "%s occupancy %s %r" % (name, shape, deep[:2])
        one = run(cb, oracle, monkeypatch, key, windows, points, "binned", (1,), carried=True)
        run(cb, oracle, monkeypatch, key, windows, points, "binned", (1, 1), carried=True)
        if shape == "every":
            run(cb, oracle, monkeypatch, key, windows, points, "binned", (50, 50))
        assert one["recorded"] + one["never_escaped"] == sum(1 for p in points if p not in P.DULL)
