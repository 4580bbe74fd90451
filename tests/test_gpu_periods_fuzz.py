"""A fixed-seed handful of random period-palette launch sequences -- step, source of c, matrix, canvas, window, iteration
control, table, tolerance, thread count and launches -- the product kernel (draw_periods_kernel, 28) against the lock-step
kernel (29): identical planes, counters (but skipped_steps) and generator states demanded, as
tests/test_gpu_bounded_fuzz.py demands them of the bounded kernels.  The shapes are small and the trials few, so they run in
this process."""

import numpy as np
import pytest

import plot_reference as plot
from period_harness import LOCKSTEP, PRODUCT, SAME, period_launches

pytestmark = pytest.mark.gpu

TRIALS, SEED = 24, 20262
STEPS = ([dict(), dict(ship=True)] + [dict(degree=d) for d in range(3, 9)] + [dict(formula=name) for name in plot.NAMES])
# fixed c with bounded orbits under the reference's step; under the other steps whatever they give
FIXED = [(-1.0, 0.0), (-0.123, 0.745), (0.0, 0.0), (0.25, 0.0), (-0.1, 0.1), (-1.75, 0.0), (0.3, 0.5)]


def trial(rng):
    kw = dict(STEPS[rng.integers(len(STEPS))])
    if rng.random() < 0.5:
        kw["c"] = FIXED[rng.integers(len(FIXED))]
    kind = rng.integers(3)
    kw["projection"] = (plot.IDENTITY, plot.ZR_CR, rng.normal(size=(2, 4)))[kind]
    lo = rng.uniform(-2.5, 0.5, size=2)
    size = rng.uniform(0.2, 4.0, size=2)
    kw["box"] = (float(lo[0]), float(lo[0] + size[0]), float(lo[1]), float(lo[1] + size[1]))
    kw["w"], kw["h"] = int(rng.integers(1, 100)), int(rng.integers(1, 100))
    kw["max_iter"] = int(rng.choice([0, 1, 12, 60, 119, 120, 121, 180, 241, 360, int(rng.integers(2, 700))]))
    kw["min_iter"] = int(rng.integers(0, 50))
    kw["threads"] = int(rng.choice([1, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 700))]))
    kw["launches"] = tuple(int(v) for v in rng.integers(1, 25, size=rng.integers(1, 4)))
    n_entries = int(rng.choice([2, 3, 13, 61, 256, 1024, int(rng.integers(2, 1025))]))
    lut = rng.integers(0, 1 << 24, size=n_entries, dtype=np.uint32)
    lut[rng.random(n_entries) < 0.3] = 0  # entries that are not replayed
    eps = float(rng.choice([0.0, 2.0 ** -66, 1e-20, 2.0 ** -20, 2.0 ** 10]))
    return lut, eps, kw


def test_random_period_launches_product_kernel_equals_lockstep_kernel(cb):
    rng = np.random.default_rng(SEED)
    skipped = plotted = 0
    for n in range(TRIALS):
        lut, eps, kw = trial(rng)
        hist, cnt, kernel, states = period_launches(cb, cb.CB_KERNEL_DEFAULT, lut, eps, **kw)
        lhist, lcnt, lkernel, lstates = period_launches(cb, cb.CB_KERNEL_SIMPLE, lut, eps, **kw)
        where = (n, len(lut), eps, {k: v for k, v in kw.items() if k != "projection"}, np.asarray(kw["projection"]).tolist())
        assert (kernel, lkernel) == (PRODUCT, LOCKSTEP), where
        assert cnt["status"] == 0 and lcnt["status"] == 0, where
        assert {k: cnt[k] for k in SAME} == {k: lcnt[k] for k in SAME}, where
        assert np.array_equal(hist, lhist) and np.array_equal(states, lstates), where
        assert int(hist.sum()) == cnt["increments"] and lcnt["skipped_steps"] == 0, where
        assert cnt["replay_steps"] == max(kw["max_iter"], 0) * cnt["recorded"] and cnt["rejected"] == 0, where
        skipped += cnt["skipped_steps"] > 0
        plotted += cnt["increments"] > 0
    print("periods fuzz: %d trials (%d with skipped_steps > 0, %d with increments > 0)" % (TRIALS, skipped, plotted))
    # (the restatement, tests/period_reference.c, run on these trials: 17 with steps skipped -- a cycle compressed or a zero
    # entry not replayed --, 12 with a point on the canvas)
    assert skipped >= 15 and plotted >= 10
