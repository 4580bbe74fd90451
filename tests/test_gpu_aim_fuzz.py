"""24 random aimed renders -- kind, step, source of c, matrix, window, level, dilation, launches -- probe then draw, the
product kernels (30) against the lock-step kernel (31): mask, list, histogram, generator states and counters (all but
skipped_steps).  The sequences are a pure function of the seed below; what each is, is printed."""

import numpy as np
import pytest

import aim_reference as aim
import plot_reference as plot
from aim_harness import LOCKSTEP, PRODUCT, bits, gpu_draw, gpu_probe
from device_launches import SAME
from test_aim_host import STEP_IDS, STEPS

pytestmark = pytest.mark.gpu

AXES = ("zr", "zi", "cr", "ci")


def sequence(index):
    rng = np.random.default_rng(20261020 + index)
    step = int(rng.integers(0, len(STEPS)))
    kw = dict(STEPS[step], bounded=bool(rng.integers(0, 2)))
    if rng.integers(0, 2):
        kw["c"] = (float(rng.choice([0.1, -1.0, 0.0, 0.25])), float(rng.choice([0.1, 0.0, -0.2])))
    x, y = rng.choice(4, 2, replace=False)
    p = plot.plane(AXES[x], AXES[y])
    if rng.integers(0, 2):
        a, b = rng.choice(4, 2, replace=False)
        p = plot.rotate(p, AXES[a], AXES[b], float(rng.uniform(-180.0, 180.0)))
    lo_u, lo_v = rng.uniform(-1.5, 0.5, 2)
    kw.update(projection=p, box=(float(lo_u), float(lo_u + rng.uniform(0.3, 1.5)), float(lo_v), float(lo_v + rng.uniform(0.3, 1.5))),
              level=int(rng.integers(4, 9)), dilate=int(rng.integers(0, 3)), threads=int(rng.integers(1, 1200)),
              max_iter=int(rng.choice([0, 7, 60, 130, 500])), min_iter=int(rng.choice([0, 2, 20])),
              w=int(rng.integers(1, 80)), h=int(rng.integers(1, 80)),
              probe=tuple(int(v) for v in rng.integers(1, 12, rng.integers(1, 4))),
              draw=tuple(int(v) for v in rng.integers(1, 30, rng.integers(1, 4))))
    return STEP_IDS[step], kw


@pytest.mark.parametrize("index", range(24))
def test_random_sequence_product_equals_lockstep(cb, index):
    step, kw = sequence(index)
    print(index, step, {k: (np.round(v, 3).tolist() if k == "projection" else v) for k, v in kw.items()})
    product, lockstep = gpu_probe(cb, 0, **kw), gpu_probe(cb, 1, **kw)
    assert (product[2], lockstep[2]) == (PRODUCT, LOCKSTEP)
    assert np.array_equal(product[0], lockstep[0]) and np.array_equal(product[3], lockstep[3])
    assert product[1]["status"] == lockstep[1]["status"] == 0
    assert {k: product[1][k] for k in SAME} == {k: lockstep[1][k] for k in SAME}, (product[1], lockstep[1])
    assert product[1]["increments"] == 0 and lockstep[1]["skipped_steps"] == 0
    cells = cb.focus_cells(kw["level"], product[0], kw["dilate"])
    print("marked", bits(product[0]), "listed", len(cells), product[1])
    if len(cells) == 0:
        cells = np.array([0, (4 << kw["level"]) ** 2 - 1], dtype=np.uint32)  # nothing marked: a planted list, the grid's corners
    product, lockstep = gpu_draw(cb, 0, cells, **kw), gpu_draw(cb, 1, cells, **kw)
    assert (product[2], lockstep[2]) == (PRODUCT, LOCKSTEP)
    assert np.array_equal(product[0], lockstep[0]) and np.array_equal(product[3], lockstep[3])
    assert product[1]["status"] == lockstep[1]["status"] == 0
    assert {k: product[1][k] for k in SAME} == {k: lockstep[1][k] for k in SAME}, (product[1], lockstep[1])
    assert int(product[0].sum()) == product[1]["increments"] and lockstep[1]["skipped_steps"] == 0
    print(product[1])
