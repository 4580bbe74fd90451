"""The anti-Buddhabrot (CB_KERNEL_FLAG_ANTI) on the GPU, byte for byte:

  1. the lock-step kernel (draw_anti_simple_kernel) against the CPU restatement (tests/anti_reference.c);
  2. the cycle-compressed product kernel (draw_anti_kernel) against the lock-step kernel on the same generator states;
  3. one renderer-sized launch against the restatement (counters past 2^32);
  4. a renderer that switches between normal and anti passes against the three renders done separately;
  5. the CLI: --anti's PGM against the restatement, and true resume with -s and --rng-state.
"""

import os

import numpy as np
import pytest

import anti_reference as anti
from device_launches import SAME, SQUARE, Launches, assert_same, gpu_run as run, omp_threads  # noqa: F401 (the edge suite's too)
from plot_harness import exe  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

PRODUCT, LOCKSTEP = 4, 5


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return anti.load(tmp_path_factory.mktemp("anti_ref"))


def gpu_anti(cb, w, h, box, max_iter, threads, passes, base, ship=False, *, seed=None, first=0, launches=None,
             min_iter=20, flags=0, hist0=None, counters0=None, no_counters=False, workspace=None, carry=None):
    """One launch of `passes` reference passes on fresh generators (seed 1337, subsequences [0, threads)) -> (u64 hist
    [h, w], counters dict, cb_debug_last_draw_kernel, generator states as u32 planes).
    seed, first: other generators; launches: samples per thread of each launch, one after another on the same states,
    instead of one of passes x 50; flags: OR-ed into the variant; hist0 (u64 [h, w]) and counters0 (one u64 per counter):
    what the buffers hold before; no_counters: d_counters = NULL (the counters come back as zeros); workspace = (torch
    buffer, bytes) and carry (torch buffer): passed to every launch."""
    seq = Launches(cb, cb.FractalDimensions.make(w, h, *box), threads, hist0=hist0, seed=seed, first=first,
                   counters0=counters0, no_counters=no_counters, workspace=workspace or 0, carry=carry)
    variant = base | cb.CB_KERNEL_FLAG_ANTI | (cb.CB_KERNEL_FLAG_BURNING_SHIP if ship else 0) | flags
    launches = [passes * cb.CB_SAMPLES_PER_THREAD] if launches is None else launches
    return seq.launches(cb.draw_buddhabrot, launches, variant, flush=False,  # an anti launch defers nothing
                        iterations=cb.IterationControl(max_iter, min_iter)).read()


CANVASES = {
    "square": (256, 256, SQUARE, False),
    "zoom": (300, 200, (-1.9, -0.7, -0.45, 0.35), False),  # deltas 0.004, 0.004: not powers of two
    "ship": (256, 256, SQUARE, True),
}


@pytest.mark.parametrize("threads", [4096, 4000])
@pytest.mark.parametrize("max_iter", [1, 2, 100, 1000])
@pytest.mark.parametrize("canvas", list(CANVASES))
def test_lockstep_anti_equals_the_restatement(cb, ref, canvas, max_iter, threads):
    w, h, box, ship = CANVASES[canvas]
    hist, cnt, kernel, _ = gpu_anti(cb, w, h, box, max_iter, threads, 2, cb.CB_KERNEL_SIMPLE, ship)
    assert kernel == LOCKSTEP
    want, wc = anti.render(ref, w, h, max_iter, threads, 2, box=box, ship=ship, omp_threads=omp_threads())
    assert cnt["skipped_steps"] == 0
    assert_same((hist, cnt), (want, wc))
    assert int(hist.sum()) == cnt["increments"]


@pytest.mark.parametrize(
    "w,h,box,max_iter,threads,ship",
    [
        (256, 256, SQUARE, 20000, 4096, False),
        (300, 200, (-1.9, -0.7, -0.45, 0.35), 20000, 4000, False),
        (256, 256, SQUARE, 5000, 1337, True),
        (1, 1, (-1.5, 0.5, -1.0, 1.0), 3000, 4096, False),
    ],
    ids=["m20000", "ragged_zoom", "ship_ragged", "one_pixel"],
)
def test_product_anti_equals_lockstep(cb, w, h, box, max_iter, threads, ship):
    p_hist, p_cnt, p_kernel, p_states = gpu_anti(cb, w, h, box, max_iter, threads, 2, cb.CB_KERNEL_DEFAULT, ship)
    l_hist, l_cnt, l_kernel, l_states = gpu_anti(cb, w, h, box, max_iter, threads, 2, cb.CB_KERNEL_SIMPLE, ship)
    assert (p_kernel, l_kernel) == (PRODUCT, LOCKSTEP)
    assert_same((p_hist, p_cnt), (l_hist, l_cnt))
    assert np.array_equal(p_states, l_states)  # both advance every generator by the same samples
    assert p_cnt["skipped_steps"] > 0 and l_cnt["skipped_steps"] == 0  # the cycles were compressed
    assert p_cnt["skipped_steps"] < p_cnt["iterate_steps"] + p_cnt["replay_steps"]


def test_renderer_sized_anti_launch(cb, ref):
    """262144 threads x 128 passes (one fused launch of cb_renderer), 1024^2, M = 200: the counters pass 2^32."""
    w = h = 1024
    dims = cb.FractalDimensions.make(w, h)
    with cb.Renderer(dims, cb.IterationControl(200, 20), device=0, n_threads=cb.CB_DEFAULT_THREADS) as r:
        r.render_passes(128, cb.CB_KERNEL_DEFAULT | cb.CB_KERNEL_FLAG_ANTI)
        assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
    want, wc = anti.render(ref, w, h, 200, cb.CB_DEFAULT_THREADS, 128, omp_threads=omp_threads())
    assert_same((hist.reshape(h, w), cnt), (want, wc))
    assert cnt["iterate_steps"] > 2 ** 32 and cnt["increments"] > 2 ** 32
    assert int(hist.sum()) == cnt["increments"]


def test_renderer_switches_between_normal_and_anti_passes(cb, ref, oracle):
    """Normal (workspace, carry), anti (direct atomics), normal again on one renderer == the three renders done one
    after another on the same generators."""
    w = h = 256
    threads, m, c = 4096, 500, 20
    dims = cb.FractalDimensions.make(w, h)
    with cb.Renderer(dims, cb.IterationControl(m, c), device=0, n_threads=threads) as r:
        r.render_passes(2)
        r.render_passes(2, cb.CB_KERNEL_DEFAULT | cb.CB_KERNEL_FLAG_ANTI)
        r.render_passes(2)
        hist = r.read_histogram().reshape(h, w)
        cnt = r.read_counters().as_dict()
    st = oracle.init_states(1337, 0, threads)
    h1, c1 = oracle.render(w, h, m, c, threads, 2, states=st, omp_threads=omp_threads())
    h2, c2 = anti.render(ref, w, h, m, threads, 2, states=st, omp_threads=omp_threads())
    h3, c3 = oracle.render(w, h, m, c, threads, 2, states=st, omp_threads=omp_threads())
    assert cnt["status"] == 0
    assert cnt["samples"] == c1["samples"] + c2["samples"] + c3["samples"]
    assert cnt["increments"] == c1["increments"] + c2["increments"] + c3["increments"]
    assert np.array_equal(hist, h1 + h2 + h3)


def test_cli_anti_image_equals_the_restatement(exe, ref, oracle, tmp_path):
    out = str(tmp_path / "anti.pgm")
    r = run(exe, "--anti", "-w", "256", "-h", "256", "-m", "300", "--passes", "3", "-o", out)
    assert r.returncode == 0, r.stdout + r.stderr
    want, _ = anti.render(ref, 256, 256, 300, 512 * 512, 3, omp_threads=omp_threads())
    gray, _, _ = oracle.set_grayscale_pixels(want, 1.0)
    with open(out, "rb") as f:
        assert f.read() == oracle.encode_pgm(gray)


def test_cli_anti_true_resume(exe, tmp_path):
    buf, side = str(tmp_path / "a.bin"), str(tmp_path / "a.rng")
    common = ["--anti", "-w", "300", "-h", "200", "-m", "200", "-o", os.devnull, "-s", buf, "--rng-state", side]
    assert run(exe, "--passes", "2", *common).returncode == 0
    r2 = run(exe, "--passes", "1", *common)
    assert r2.returncode == 0 and "Continuing the sample stream after 2 passes." in r2.stdout, r2.stdout
    one_buf, one_side = str(tmp_path / "b.bin"), str(tmp_path / "b.rng")
    r3 = run(exe, "--passes", "3", "--anti", "-w", "300", "-h", "200", "-m", "200", "-o", os.devnull, "-s", one_buf,
             "--rng-state", one_side)
    assert r3.returncode == 0
    with open(buf, "rb") as a, open(one_buf, "rb") as b:
        assert a.read() == b.read()
    with open(side, "rb") as a, open(one_side, "rb") as b:
        assert a.read() == b.read()
