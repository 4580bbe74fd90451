"""The period-palette render (include/cudabrot_amd.h, "Period-palette render") without a GPU: the CPU restatement
(tests/period_reference.c) evaluated twice -- naively, the definition: iterate to M, continue J steps for the period, replay
M points -- and compressed, on the product kernel's schedule: chunks of 60 steps, the refined Brent saves, the walk of rem
steps from z_s to the probe, the search, a zero entry not replayed -- gives the same three planes and counters bit for bit,
for every step family and both sources of c, at the schedule's edges in M, for every J and eps.  That is DESIGN.md 4.22's
proof sentence, run.  Then the four consequences of the definition against the bounded render's restatement, the ABI's
names, and what the entry point refuses without touching a device."""

import ctypes as C
import math
import os

import numpy as np
import pytest

import bounded_reference as bounded
import period_reference as period
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
INVALID = 1  # hipErrorInvalidValue
EPS = (0.0, 2.0 ** -66, 2.0 ** 10)
JS = (1, 2, 7, 255, 1023)


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return period.load(tmp_path_factory.mktemp("period_ref"))


def both(pref, lut, max_iter=MAX, **kw):
    out = []
    for mode in (period.NAIVE, period.COMPRESSED):
        extra = {}
        hist, cnt = period.draw(pref, W, H, max_iter, THREADS, LAUNCHES, lut, mode=mode, omp_threads=omp_threads(),
                                extra=extra, **kw)
        out.append((hist, cnt, extra))
    return out


def same_but_the_search(ne, ce):
    """The classes are the schedule's, whatever the mode; the search's steps are the mode's own."""
    return {k: ne[k] for k in period.CLASSES + ("escaped",)} == {k: ce[k] for k in period.CLASSES + ("escaped",)}


# ---- 1. naive == compressed ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("step", list(STEPS))
def test_the_compressed_evaluation_equals_the_naive_one(pref, step, source):
    projection = plot.HOLOGRAM if step in ("power_3", "celtic") else plot.ZR_CR if step == "reference" else plot.IDENTITY
    lut = period.gradient_table(256)
    (nh, nc, ne), (ch, cc, ce) = both(pref, lut, c=SOURCES[source], projection=projection, box=CROP, **STEPS[step])
    assert nh.shape == (3, H, W) and np.array_equal(nh, ch)
    assert {k: nc[k] for k in SAME} == {k: cc[k] for k in SAME} and same_but_the_search(ne, ce)
    assert nc["skipped_steps"] == 0 < cc["skipped_steps"]  # and the compression was used
    assert ne["escaped"] > 0 and ne["cycle_period"] > 0 and nc["increments"] > 0
    # the counters' identities
    samples = THREADS * sum(LAUNCHES)
    bounded_samples = sum(ne[k] for k in ("cycle_period", "cycle_none", "tol_period", "tol_none"))
    assert nc["samples"] == samples == ne["escaped"] + bounded_samples
    assert nc["rejected"] == 0 and nc["too_fast"] == ne["escaped"]
    assert nc["never_escaped"] == nc["recorded"] == bounded_samples and nc["replay_steps"] == MAX * nc["recorded"]
    assert int(nh.sum()) == nc["increments"]
    # the search: at most J steps per bounded sample in the definition; the compressed walk adds its rem steps
    assert bounded_samples <= ne["search_steps"] <= 255 * bounded_samples and ce["search_steps"] >= ne["search_steps"]


@pytest.mark.parametrize("max_iter", [0, 1, 11, 12, 13, 59, 60, 61, 119, 120, 121, 180, 181, 239, 240])
@pytest.mark.parametrize("source", list(SOURCES))
def test_the_two_evaluations_agree_at_the_schedules_edges(pref, max_iter, source):
    c = None if source == "sampled" else (-1.0, 0.0)
    for j in JS:
        for eps in EPS:
            # a table with a zero entry at an odd period and at no period: both replay decisions are taken
            lut = period.gradient_table(j + 1)
            if j >= 7:
                lut[3] = 0
            (nh, nc, ne), (ch, cc, ce) = both(pref, lut, max_iter=max_iter, c=c, box=CROP, eps=eps)
            where = (max_iter, j, eps)
            assert np.array_equal(nh, ch), where
            assert {k: nc[k] for k in SAME} == {k: cc[k] for k in SAME} and same_but_the_search(ne, ce), where
            assert nc["replay_steps"] == max_iter * nc["recorded"] and int(nh.sum()) == nc["increments"], where
            if max_iter < 120:  # the first comparison is at k = 120
                assert ne["cycle_period"] == ne["cycle_none"] == 0, where
                assert cc["skipped_steps"] == max_iter * ne["zero_entry"], where  # nothing but the replays not made
            if max_iter == 0:
                assert nc["recorded"] == nc["samples"] and nc["iterate_steps"] == 0 and nc["increments"] == 0, where
            if max_iter == 120:  # a match at k = M = 120: s = 60, p = 60, rem = 0: the probe is z_s itself
                assert ne["rem_zero"] == ne["cycle_period"] + ne["cycle_none"] > 0, where
            if max_iter == 181:
                assert ne["rem_zero"] == 0 < ne["cycle_period"] + ne["cycle_none"], where


def test_the_inputs_reach_every_class(pref):
    total = dict.fromkeys(period.CLASSES, 0)
    lut = period.gradient_table(256)
    lut[2] = 0  # the period-2 bulb is not replayed
    for kw in (dict(), dict(max_iter=120), dict(lut=period.gradient_table(2)), dict(c=(-0.123, 0.745), max_iter=130)):
        kw = dict(kw)
        table = kw.pop("lut", lut)
        _, (_, _, extra) = both(pref, table, **kw)
        print(kw, extra)
        for k in total:
            total[k] += extra[k]
    for k, v in total.items():
        assert v > 0, (k, total)


# ---- 2. the consequences of the definition, against the bounded render's restatement -------------------------------------


@pytest.fixture(scope="module")
def bounded_want(pref):
    def get(**kw):
        extra = {}
        hist, cnt = bounded.draw(pref, W, H, MAX, THREADS, LAUNCHES, omp_threads=omp_threads(), extra=extra, **kw)
        return hist, cnt

    return get


@pytest.mark.parametrize("kw", [dict(box=CROP), dict(projection=plot.ZR_CR), dict(c=(-0.123, 0.745)), dict(degree=3, box=CROP)],
                         ids=["reference", "zr_cr", "rabbit", "cubic"])
def test_the_constant_table_is_the_bounded_render_three_times(pref, bounded_want, kw):
    want, wc = bounded_want(**kw)
    for mode in (period.NAIVE, period.COMPRESSED):
        for n in (2, 256):
            hist, cnt = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, period.constant_table(n), mode=mode,
                                    omp_threads=omp_threads(), **kw)
            for j in range(3):
                assert np.array_equal(hist[j], want)
            assert cnt["increments"] == 3 * wc["increments"] > 0
            assert {k: cnt[k] for k in SAME if k != "increments"} == {k: wc[k] for k in SAME if k != "increments"}
    # and the compressed skipped_steps is the bounded render's: nothing is left unreplayed for its colour
    _, bc = bounded.draw(pref, W, H, MAX, THREADS, LAUNCHES, mode=bounded.COMPRESSED, omp_threads=omp_threads(), **kw)
    assert cnt["skipped_steps"] == bc["skipped_steps"] > 0


@pytest.mark.parametrize("mode", [period.NAIVE, period.COMPRESSED], ids=["naive", "compressed"])
def test_the_one_hot_tables_sum_to_the_bounded_render_and_combine_linearly(pref, bounded_want, mode):
    n = 8  # J = 7: periods 0 .. 7
    kw = dict(box=CROP)
    want, wc = bounded_want(**kw)
    parts, skipped, zero = [], [], []
    for k in range(n):
        extra = {}
        hist, cnt = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, period.one_hot(n, k), mode=mode,
                                omp_threads=omp_threads(), extra=extra, **kw)
        assert not hist[1].any() and not hist[2].any()
        assert {x: cnt[x] for x in SAME if x != "increments"} == {x: wc[x] for x in SAME if x != "increments"}
        parts.append(hist[0])
        skipped.append(cnt["skipped_steps"])
        zero.append(extra["zero_entry"])
    assert np.array_equal(sum(parts), want)
    assert sum(1 for p in parts if p.any()) >= 4  # periods 0, 1, 2 and another
    assert sum(zero) == (n - 1) * wc["recorded"]  # every bounded sample has one period
    if mode == period.NAIVE:
        assert not any(skipped)
    lut = period.gradient_table(n)
    hist, cnt = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, lut, mode=mode, omp_threads=omp_threads(), **kw)
    for j in range(3):
        weights = [(int(e) >> (8 * j)) & 255 for e in lut]
        assert np.array_equal(hist[j], sum(np.uint64(w) * p for w, p in zip(weights, parts)))


def test_a_wide_eps_gives_every_bounded_sample_of_the_reference_step_period_one(pref, bounded_want):
    want, wc = bounded_want(box=CROP)
    for n in (2, 256):
        extra = {}
        hist, cnt = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, period.one_hot(n, 1), eps=2.0 ** 10, box=CROP,
                                omp_threads=omp_threads(), extra=extra)
        assert np.array_equal(hist[0], want) and cnt["increments"] == wc["increments"] > 0
        assert extra["cycle_none"] == extra["tol_none"] == extra["zero_entry"] == 0
        assert extra["search_steps"] == wc["recorded"]  # one step each


def test_eps_zero_is_an_exact_return_and_needs_more_steps_than_the_default(pref):
    lut = period.one_hot(256, 0)  # plane 0: the samples without a period
    exact, tolerant = {}, {}
    he, _ = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, lut, eps=0.0, box=CROP, omp_threads=omp_threads(), extra=exact)
    ht, _ = period.draw(pref, W, H, MAX, THREADS, LAUNCHES, lut, box=CROP, omp_threads=omp_threads(), extra=tolerant)
    none_exact = exact["cycle_none"] + exact["tol_none"]
    none_tolerant = tolerant["cycle_none"] + tolerant["tol_none"]
    assert none_exact > none_tolerant > 0 and int(he.sum()) > int(ht.sum()) > 0
    assert exact["search_steps"] > tolerant["search_steps"]


# ---- 3. the header and the package ---------------------------------------------------------------------------------------


def test_the_abi_names_the_render(cb):
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    assert text.index("---- Bounded render:") < text.index("---- Period-palette render:") < text.index("---- Renderer:")
    start = text.index("---- Period-palette render:")
    section = text[start:text.index("---- Renderer:", start)]
    for phrase in ("2 <= n_entries <= CB_PERIOD_MAX_ENTRIES (1024)", "J = n_entries - 1", "a finite double >= 0",
                   "dr = re(z_{M+j}) - re(z_M)", "di = im(z_{M+j}) - im(z_M)", "d2 = fma(dr, dr, di * di)",
                   "least j with d2 <= eps", "a NaN compares false", "no schedule enters", "with +0 and -0 alike",
                   "adds weight_j(lut[pi]) to its pixel of plane j", "increments is the sum of the weights added",
                   "counted nowhere", "cb_palette_from_stops(stops, n, lut, n_entries)", "0x010101", "0x1p+10",
                   "#define CB_PERIOD_MAX_ENTRIES 1024", "rem = (M - s) mod p"):
        assert phrase in section, phrase
    names = ("cb_draw_buddhabrot_periods", "cb_renderer_set_period_palette", "cb_renderer_period_palette",
             "cb_renderer_period_palette_image")
    for name in names:
        assert name + "(" in text and name in cb.capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "28 the period-palette product kernel" in text and "29 the period-palette lock-step kernel" in text
    assert "draw_buddhabrot_periods" in cb.__all__ and callable(cb.draw_buddhabrot_periods)
    assert "CB_PERIOD_MAX_ENTRIES" in cb.__all__ and cb.CB_PERIOD_MAX_ENTRIES == 1024
    assert all(hasattr(cb.Renderer, n) for n in ("set_period_palette", "period_palette", "period_palette_image"))
    assert cb.lib.cb_abi_version() == 1  # the change only adds


# ---- 4. validation that needs no device ----------------------------------------------------------------------------------

NAN, INF = math.nan, math.inf


def call(cb, lut=4096, n_entries=256, eps=2.0 ** -66, *, variant=None, julia=None, projection=None, hist=4096, states=4096):
    """cb_draw_buddhabrot_periods with pointers that are never followed: a launch of no threads launches nothing, so an
    accepted call returns 0 without touching a device."""
    dims = cb.FractalDimensions.make(16, 16)
    it = cb.IterationControl(100, 20)
    p = None if projection is False else (C.c_double * 8)(*(cb.IDENTITY_PROJECTION if projection is None else projection))
    c = None if julia is None else (C.c_double * 2)(*julia)
    return cb.lib.cb_draw_buddhabrot_periods(C.byref(dims), hist, C.byref(it), p, c, lut, n_entries, eps, states, 0, 50,
                                             None, cb.CB_KERNEL_SIMPLE if variant is None else variant, None)


def test_a_valid_call_is_accepted(cb):
    for n in (2, 3, 256, 1024):
        assert call(cb, n_entries=n) == 0, n
    for eps in (0.0, 5e-324, 2.0 ** -66, 2.0 ** 10, 1.7976931348623157e308):
        assert call(cb, eps=eps) == 0, eps
    assert call(cb, julia=(-1.0, 0.0)) == 0 and call(cb, julia=(2.0, -2.0)) == 0
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        for flag in (0, cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_POWER(8), cb.CB_KERNEL_FORMULA("tricorn"), cb.CB_KERNEL_FORMULA(5),
                     cb.CB_KERNEL_FLAG_BURNING_SHIP):
            assert call(cb, variant=base | flag) == 0, (base, flag)


def test_what_the_definition_and_the_bounded_draw_refuse_is_refused(cb):
    assert call(cb, lut=None) == INVALID  # no table
    for n in (0, 1, 1025, 4096, 0xFFFFFFFF):
        assert call(cb, n_entries=n) == INVALID, n
    for eps in (-0.0 - 5e-324, -1.0, -INF, INF, NAN):
        assert call(cb, eps=eps) == INVALID, eps
    assert call(cb, projection=(1, 0, 0, 0, 0, NAN, 0, 0)) == INVALID and call(cb, projection=False) == INVALID
    assert call(cb, projection=(INF, 0, 0, 0, 0, 1, 0, 0)) == INVALID
    for c in ((2.5, 0.0), (0.0, -2.0000001), (NAN, 0.0), (0.0, NAN), (0.0, INF)):
        assert call(cb, julia=c) == INVALID, c
    ship, power3, tricorn = cb.CB_KERNEL_FLAG_BURNING_SHIP, cb.CB_KERNEL_POWER(3), cb.CB_KERNEL_FORMULA(1)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        for flag in (cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_FLAG_ANTI | ship, power3 | ship,
                     tricorn | ship, tricorn | power3, 2 << 12, 9 << 12, 6 << 16):
            assert call(cb, variant=base | flag) == INVALID, (base, flag)
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_TIMED | ship):
        assert call(cb, variant=variant) == INVALID, variant
    assert call(cb, hist=None) == INVALID and call(cb, states=None) == INVALID
    # the renderer's calls on no renderer: refused, and the getter leaves its outputs alone
    table = np.ascontiguousarray(period.gradient_table(8), dtype=np.uint32)
    assert cb.lib.cb_renderer_set_period_palette(None, table.ctypes.data, 8, 0.0) == INVALID
    n, eps = C.c_uint32(77), C.c_double(0.5)
    assert cb.lib.cb_renderer_period_palette(None, C.byref(n), C.byref(eps)) == 0 and n.value == 77 and eps.value == 0.5
    assert cb.lib.cb_renderer_period_palette_image(None, 1.0, 0, None, None, None) == INVALID


def test_stops_make_the_table_with_k_read_as_a_period(cb):
    lut = cb.palette_from_stops([(1, 255, 0, 0), (2, 0, 255, 0), (4, 0, 0, 255)], 5)
    assert lut.tolist()[:3] == [0x0000FF, 0x0000FF, 0x00FF00] and lut[4] == 0xFF0000  # entry 0: the first stop's colour
    assert cb.lib.cb_palette_from_stops is not None and len(lut) == 5
