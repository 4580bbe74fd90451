"""The bounded render (include/cudabrot_amd.h, "Bounded render") without a GPU: the CPU restatement
(tests/bounded_reference.c) evaluated twice -- naively, every one of the M points of a bounded orbit with weight 1, and
compressed, the transient once plus one weighted period, on the product kernel's schedule (chunks of 60 steps, the refined
Brent saves) -- gives the same histogram and counters bit for bit, for every step family and both sources of c.  That is
DESIGN.md 4.21's extension of 4.9's proof, run.  And the counters' identities, the ABI's names, and that the inputs reach
both branches."""

import os

import numpy as np
import pytest

import bounded_reference as bounded
import plot_reference as plot
from device_launches import SAME, omp_threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX, THREADS, LAUNCHES = 32, 24, 500, 200, (3, 20, 1)
CROP = (-1.5, 0.7, -0.9, 1.1)
STEPS = {"reference": dict(), "ship": dict(ship=True)}
STEPS.update({"power_%d" % d: dict(degree=d) for d in range(3, 9)})
STEPS.update({name: dict(formula=name) for name in plot.NAMES})
# a c near 0 has an attracting fixed point under every step: bounded orbits that land on an exact cycle
SOURCES = {"sampled": None, "fixed": (-0.1, 0.1)}


@pytest.fixture(scope="module")
def bref(tmp_path_factory):
    return bounded.load(tmp_path_factory.mktemp("bounded_ref"))


def both(bref, max_iter=MAX, **kw):
    out = []
    for mode in (bounded.NAIVE, bounded.COMPRESSED):
        extra = {}
        hist, cnt = bounded.draw(bref, W, H, max_iter, THREADS, LAUNCHES, mode=mode, omp_threads=omp_threads(), extra=extra,
                                 **kw)
        out.append((hist, cnt, extra))
    return out


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("step", list(STEPS))
def test_the_compressed_evaluation_equals_the_naive_one(bref, step, source):
    projection = plot.HOLOGRAM if step in ("power_3", "celtic") else plot.ZR_CR if step == "reference" else plot.IDENTITY
    (nh, nc, ne), (ch, cc, ce) = both(bref, c=SOURCES[source], projection=projection, box=CROP, **STEPS[step])
    assert np.array_equal(nh, ch)
    assert {k: nc[k] for k in SAME} == {k: cc[k] for k in SAME} and ne == ce
    assert nc["skipped_steps"] == 0 < cc["skipped_steps"]  # and the compression was used
    assert ne["escaped"] > 0 and ne["cycles"] > 0 and nc["increments"] > 0
    # the counters' identities
    samples = THREADS * sum(LAUNCHES)
    assert nc["samples"] == samples == ne["escaped"] + ne["cycles"] + ne["no_cycle"]
    assert nc["rejected"] == 0 and nc["too_fast"] == ne["escaped"]
    assert nc["never_escaped"] == nc["recorded"] == ne["cycles"] + ne["no_cycle"]
    assert nc["replay_steps"] == MAX * nc["recorded"] == ne["in_canvas"] + ne["off_canvas"]
    assert int(nh.sum()) == nc["increments"] == ne["in_canvas"]
    assert MAX * nc["recorded"] + nc["too_fast"] <= nc["iterate_steps"] <= MAX * samples


@pytest.mark.parametrize("max_iter", [0, 1, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 181, 239, 240])
@pytest.mark.parametrize("source", list(SOURCES))
def test_the_two_evaluations_agree_at_the_schedules_edges(bref, max_iter, source):
    c = None if source == "sampled" else (-1.0, 0.0)
    (nh, nc, ne), (ch, cc, ce) = both(bref, max_iter=max_iter, c=c, box=CROP)
    assert np.array_equal(nh, ch) and {k: nc[k] for k in SAME} == {k: cc[k] for k in SAME} and ne == ce
    assert nc["replay_steps"] == max_iter * nc["recorded"] and int(nh.sum()) == nc["increments"]
    if max_iter < 120:  # the first comparison is at k = 120
        assert ne["cycles"] == 0 and cc["skipped_steps"] == 0
    if max_iter == 0:
        assert nc["recorded"] == nc["samples"] and nc["iterate_steps"] == 0 and nc["increments"] == 0
    if max_iter == 120:  # a match at k = M = 120: s = 60, p = 60, every cycle point once, nothing saved but nothing wrong
        assert ne["cycles"] == ne["at_m"] == ne["rem_zero"] > 0
    if max_iter == 180:
        assert ne["rem_zero"] == ne["cycles"] > 0 and cc["skipped_steps"] > 0
    if max_iter == 181:
        assert ne["rem_zero"] == 0 < ne["cycles"]


def test_a_sampled_c_reaches_every_branch_and_a_fixed_c_has_no_slow_orbits_but_at_a_small_max(bref):
    for kw in (dict(projection=plot.ZR_CR), dict(ship=True), dict(degree=3), dict(formula="tricorn")):
        _, (_, _, extra) = both(bref, box=CROP, **kw)
        for key in ("escaped", "cycles", "no_cycle", "both_weights", "in_canvas", "off_canvas"):
            assert extra[key] > 0, (kw, extra)
    _, (_, _, extra) = both(bref, c=(-1.0, 0.0))
    assert extra["no_cycle"] == 0 < extra["cycles"] == extra["both_weights"]
    _, (_, _, extra) = both(bref, max_iter=130, c=(-0.123, 0.745))  # the rabbit's slowest orbits are not yet exact at k = 60
    assert extra["no_cycle"] > 0 and extra["cycles"] > 0


def test_the_identity_with_a_sampled_c_is_the_anti_buddhabrot(bref, tmp_path):
    import anti_reference as anti

    aref = anti.load(tmp_path)
    for ship in (False, True):
        want, wc = anti.render(aref, W, H, MAX, THREADS, 1, box=CROP, ship=ship, mode=anti.NAIVE, samples_per_thread=24)
        hist, cnt = bounded.draw(bref, W, H, MAX, THREADS, (24,), ship=ship, box=CROP)
        assert np.array_equal(hist, want) and {k: cnt[k] for k in SAME} == {k: wc[k] for k in SAME}
        assert cnt["recorded"] > 0


def test_the_abi_names_the_render(cb):
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert "Bounded render" in text
    for name in ("cb_draw_buddhabrot_bounded", "cb_renderer_set_bounded", "cb_renderer_bounded"):
        assert name + "(" in text and name in cb.capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "draw_buddhabrot_bounded" in cb.__all__ and callable(cb.draw_buddhabrot_bounded)
    assert "26 the bounded product kernel" in text and "27 the bounded lock-step kernel" in text
