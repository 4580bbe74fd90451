"""The anti-Buddhabrot kernels (draw_anti.hip) against the DEFINITION, at the M where the product kernel decides something.

tests/test_gpu_anti.py compares the product kernel with the lock-step kernel at M >= 3000 and the lock-step kernel with
the restatement's compressed mode, which follows the kernel's own schedule.  Here both kernels are compared with the naive
mode of tests/anti_reference.c -- iterate to M, replay M points with weight 1 -- at anti_reference.EDGE_M: rounds of 12
steps, chunks of 60, cycles found at k == M (120, 180, 240: `end = M - 1, q = 1, rem = 0`), a weight split with a
remainder (M % 60 != 0), and M <= 0.  tests/test_anti_host.py asserts, from the restatement's census, that the default
sample stream meets each of those branches a thousand times and more.  Then the launch shape (several launches, ragged
thread counts, other generators, degenerate canvases) and the sentences of include/cudabrot_amd.h about an anti launch.
"""

import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import anti_reference as anti
from conftest import read_state_file
from device_launches import SQUARE, Launches, assert_same, counter_names, omp_threads, planar_states
from test_gpu_anti import CANVASES, LOCKSTEP, PRODUCT, gpu_anti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
T = 512 * 512  # the CLI's threads per rank


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return anti.load(tmp_path_factory.mktemp("anti_ref"))


def definition(ref, oracle, w, h, box, max_iter, threads, ship=False, seed=1337, first=0, samples=100):
    """One run of `samples` samples per thread -> (naive hist, naive counters, the compressed mode's skipped_steps, the
    generator states afterwards as the device's u32 planes)."""
    st = oracle.init_states(seed, first, threads)
    args = dict(box=box, ship=ship, omp_threads=omp_threads(), samples_per_thread=samples)
    hist, cnt = anti.render(ref, w, h, max_iter, threads, 1, mode=anti.NAIVE, states=st, **args)
    _, cc = anti.render(ref, w, h, max_iter, threads, 1, mode=anti.COMPRESSED, seed=seed, first_subsequence=first, **args)
    return hist, cnt, cc["skipped_steps"], planar_states(st)


def check(got, want, product):
    hist, cnt, kernel, states = got
    w_hist, w_cnt, w_skipped, w_states = want
    assert kernel == (PRODUCT if product else LOCKSTEP)
    assert_same((hist, cnt), (w_hist, w_cnt))
    assert int(hist.sum()) == cnt["increments"]
    # both follow one schedule (chunks of 60, the refined Brent saves), so the steps not executed are the same number
    assert cnt["skipped_steps"] == (w_skipped if product else 0), (cnt["skipped_steps"], w_skipped)
    assert np.array_equal(states, w_states)


# ---- B1: both kernels against the definition ----------------------------------------------------------------------

@pytest.mark.parametrize("threads", [4096, 1337])
@pytest.mark.parametrize("max_iter", anti.EDGE_M)
@pytest.mark.parametrize("canvas", list(CANVASES))
def test_both_kernels_equal_the_definition(cb, ref, oracle, canvas, max_iter, threads):
    w, h, box, ship = CANVASES[canvas]
    want = definition(ref, oracle, w, h, box, max_iter, threads, ship)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        got = gpu_anti(cb, w, h, box, max_iter, threads, 2, base, ship)
        check(got, want, base == cb.CB_KERNEL_DEFAULT)
        if max_iter <= 0:  # nothing tested, nothing added: every sample counts as not escaping
            hist, cnt = got[0], got[1]
            assert int(hist.sum()) == 0
            assert cnt["never_escaped"] == cnt["recorded"] == cnt["samples"] == threads * 100
            assert cnt["too_fast"] == cnt["iterate_steps"] == cnt["replay_steps"] == cnt["increments"] == 0
            assert cnt["skipped_steps"] == 0
    if max_iter == 120:  # a cycle found at k == M skips exactly its last replay step
        assert 1000 <= want[2] < want[1]["recorded"]


# ---- B2: launch shape ---------------------------------------------------------------------------------------------

SHAPES = {
    "one_thread": dict(threads=1),
    "threads_63": dict(threads=63),
    "threads_64": dict(threads=64),
    "threads_65": dict(threads=65),
    "threads_257": dict(threads=257),
    "seed_1_first_262144": dict(seed=1, first=262144),
    "seed_64_bit_first_2097151": dict(seed=0xdeadbeefcafe, first=2097151),
    "canvas_1x200": dict(w=1, h=200),
    "canvas_7x1": dict(w=7, h=1),
    "far_window": dict(box=(1.0, 3.0, 1.0, 2.5)),  # almost nothing lands there
    "ship_ragged": dict(threads=1337, ship=True),
}


@pytest.mark.parametrize("max_iter", [181, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_launches_of_any_shape_equal_one_run_of_the_definition(cb, ref, oracle, shape, max_iter):
    """Launches of 1, 7 and 150 samples per thread on the same generators == one run of 158 samples per thread."""
    s = dict(dict(w=256, h=256, box=SQUARE, threads=4096, ship=False, seed=1337, first=0), **SHAPES[shape])
    want = definition(ref, oracle, s["w"], s["h"], s["box"], max_iter, s["threads"], s["ship"], s["seed"], s["first"],
                      samples=158)
    got = gpu_anti(cb, s["w"], s["h"], s["box"], max_iter, s["threads"], 0, cb.CB_KERNEL_DEFAULT, s["ship"],
                   seed=s["seed"], first=s["first"], launches=[1, 7, 150])
    check(got, want, product=True)
    assert want[1]["samples"] == 158 * s["threads"]
    if shape == "far_window":
        assert want[1]["increments"] < want[1]["recorded"]  # less than a point per orbit, if any at all


@pytest.mark.parametrize("base", ["product", "lockstep"])
def test_a_launch_of_no_samples_changes_nothing(cb, oracle, base):
    hist0 = (np.arange(256 * 256, dtype=np.uint64) % 1000 + 1).reshape(256, 256)
    counters0 = np.arange(1, len(counter_names(cb)) + 1, dtype=np.uint64) * 1000
    variant = cb.CB_KERNEL_DEFAULT if base == "product" else cb.CB_KERNEL_SIMPLE
    hist, cnt, _, states = gpu_anti(cb, 256, 256, SQUARE, 181, 1337, 0, variant, hist0=hist0, counters0=counters0,
                                    launches=[0])
    assert np.array_equal(hist, hist0)
    assert list(cnt.values()) == [int(v) for v in counters0]
    assert np.array_equal(states, planar_states(oracle.init_states(1337, 0, 1337)))


# ---- B3: the contract of include/cudabrot_amd.h -------------------------------------------------------------------

def test_workspace_carry_and_drain_flag_are_ignored(cb, ref, oracle):
    """A real workspace and a carry buffer, both filled with a pattern, and CB_KERNEL_FLAG_DRAIN: the same result as
    without them, complete without cb_flush_scatter, and neither buffer is written."""
    import torch

    w, h, box, m, threads = 256, 256, SQUARE, 181, 4096
    dev = torch.device("cuda", 0)
    ws_bytes = cb.scatter_workspace_bytes(cb.FractalDimensions.make(w, h, *box), threads, 100)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    carry = torch.full((cb.carry_bytes(threads),), 0x5A, dtype=torch.uint8, device=dev)
    want = definition(ref, oracle, w, h, box, m, threads)
    plain = gpu_anti(cb, w, h, box, m, threads, 2, cb.CB_KERNEL_DEFAULT)
    for base in (cb.CB_KERNEL_DEFAULT, cb.CB_KERNEL_SIMPLE):
        got = gpu_anti(cb, w, h, box, m, threads, 2, base, flags=cb.CB_KERNEL_FLAG_DRAIN, workspace=(ws, ws_bytes),
                       carry=carry)
        check(got, want, base == cb.CB_KERNEL_DEFAULT)
        if base == cb.CB_KERNEL_DEFAULT:
            assert got[1] == plain[1]  # every counter, skipped_steps and the untouched timing fields included
        assert bool((ws == 0xA5).all()) and bool((carry == 0x5A).all())


def test_a_launch_adds_to_the_histogram_and_the_counters(cb, ref, oracle):
    w, h, box, m, threads = 300, 200, CANVASES["zoom"][2], 181, 1337
    want_hist, want_cnt, want_skipped, want_states = definition(ref, oracle, w, h, box, m, threads)
    hist0 = (np.arange(w * h, dtype=np.uint64) * 2654435761 % 100003).reshape(h, w)
    counters0 = np.arange(1, len(counter_names(cb)) + 1, dtype=np.uint64) * 1000003
    counters0[counter_names(cb).index("status")] = 0  # flags, not a count
    hist, cnt, kernel, states = gpu_anti(cb, w, h, box, m, threads, 2, cb.CB_KERNEL_DEFAULT, hist0=hist0,
                                         counters0=counters0)
    assert kernel == PRODUCT
    assert np.array_equal(hist, hist0 + want_hist)
    names = list(cnt)
    added = dict(want_cnt, skipped_steps=want_skipped, status=0)
    for k, name in enumerate(names):
        assert cnt[name] == int(counters0[k]) + added.get(name, 0), name  # the timing fields are left as they were
    assert np.array_equal(states, want_states)
    # d_counters = NULL: the same histogram
    hist_nc, cnt_nc, _, states_nc = gpu_anti(cb, w, h, box, m, threads, 2, cb.CB_KERNEL_DEFAULT, hist0=hist0,
                                             no_counters=True)
    assert np.array_equal(hist_nc, hist) and np.array_equal(states_nc, states)
    assert not any(cnt_nc.values())
    hist_ls, _, kernel_ls, _ = gpu_anti(cb, w, h, box, m, threads, 2, cb.CB_KERNEL_SIMPLE, hist0=hist0, no_counters=True)
    assert kernel_ls == LOCKSTEP and np.array_equal(hist_ls, hist)


@pytest.mark.parametrize("base", ["product", "lockstep"])
def test_min_escape_iterations_is_ignored(cb, base):
    variant = cb.CB_KERNEL_DEFAULT if base == "product" else cb.CB_KERNEL_SIMPLE
    runs = [gpu_anti(cb, 256, 256, SQUARE, 181, 1337, 2, variant, min_iter=c) for c in (0, 20, 10 ** 6)]
    assert runs[0][1]["recorded"] > 0
    for hist, cnt, kernel, states in runs[1:]:
        assert np.array_equal(states, runs[0][3])
        assert_same((hist, cnt), runs[0])
        assert cnt["skipped_steps"] == runs[0][1]["skipped_steps"]
        assert kernel == runs[0][2]


def test_variants_that_do_not_take_the_anti_flag_are_refused(cb):
    """CB_KERNEL_TIMED and CB_KERNEL_FULL_ITERATE with the flag through cb_draw_buddhabrot, and the flag with any base
    through cb_draw_buddhabrot_channels: hipErrorInvalidValue, and nothing is touched."""
    import ctypes as C

    import torch

    w = h = 64
    threads = 256
    dims = cb.FractalDimensions.make(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    # a good lock-step launch first: cb_debug_last_draw_kernel then says 5, and a refusal must leave it there
    _, _, kernel, _ = gpu_anti(cb, w, h, SQUARE, 13, threads, 1, cb.CB_KERNEL_SIMPLE)
    assert kernel == LOCKSTEP
    bufs = Launches(cb, dims, threads, planes=2)
    hist, counters, states = bufs.out.fill_(7), bufs.counters.fill_(11), bufs.states
    torch.cuda.synchronize()
    states0 = states.clone()
    it = cb.IterationControl(181, 20)
    anti_flag, ship = cb.CB_KERNEL_FLAG_ANTI, cb.CB_KERNEL_FLAG_BURNING_SHIP
    for variant in (cb.CB_KERNEL_TIMED | anti_flag, cb.CB_KERNEL_FULL_ITERATE | anti_flag,
                    cb.CB_KERNEL_TIMED | anti_flag | ship, cb.CB_KERNEL_FULL_ITERATE | anti_flag | cb.CB_KERNEL_FLAG_DRAIN):
        rc = cb.lib.cb_draw_buddhabrot(C.byref(dims), hist.data_ptr(), C.byref(it), states.data_ptr(), threads, 50,
                                       counters.data_ptr(), variant, 0, 0, 0, stream)
        assert rc == HIP_ERROR_INVALID_VALUE, (variant, rc)
        assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP
    windows = (cb.IterationControl * 2)(cb.IterationControl(181, 20), cb.IterationControl(100, 0))
    for variant in (cb.CB_KERNEL_DEFAULT | anti_flag, cb.CB_KERNEL_SIMPLE | anti_flag, cb.CB_KERNEL_TIMED | anti_flag,
                    cb.CB_KERNEL_FULL_ITERATE | anti_flag, cb.CB_KERNEL_DEFAULT | anti_flag | ship):
        for n_channels in (1, 2):
            rc = cb.lib.cb_draw_buddhabrot_channels(C.byref(dims), hist.data_ptr(), windows, n_channels,
                                                    states.data_ptr(), threads, 50, counters.data_ptr(), variant, 0, 0,
                                                    0, stream)
            assert rc == HIP_ERROR_INVALID_VALUE, (variant, n_channels, rc)
            assert cb.lib.cb_debug_last_draw_kernel() == LOCKSTEP
    torch.cuda.synchronize()
    assert bool((hist == 7).all()) and bool((counters == 11).all()) and torch.equal(states, states0)


RENDERER_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import cudabrot_amd as cb
assert cb.lib.cb_debug_knob(b"CUDABROT_AMD_PASSES_PER_LAUNCH") == b"2"
dims = cb.FractalDimensions.make(300, 200, -1.9, -0.7, -0.45, 0.35)
with cb.Renderer(dims, cb.IterationControl(181, 20), device=0, n_threads=1337) as r:
    r.render_passes(5, cb.CB_KERNEL_DEFAULT | cb.CB_KERNEL_FLAG_ANTI)
    kernel = cb.lib.cb_debug_last_draw_kernel()
    hist, states = r.read_histogram(), r.read_rng_states()
    cnt = r.read_counters().as_dict()
np.savez(sys.argv[2], hist=hist, states=states, kernel=kernel, names=list(cnt), counters=np.array(list(cnt.values()), dtype=np.uint64))
"""


def test_renderer_splits_anti_passes_into_several_launches(ref, oracle, tmp_path):
    """5 anti passes with at most 2 per launch (launches of 2, 2 and 1 pass; the knob is read once per process, hence the
    child) == one run of 5 passes of the definition."""
    out = str(tmp_path / "renderer.npz")
    env = dict(os.environ, CUDABROT_AMD_DEBUG="1", CUDABROT_AMD_PASSES_PER_LAUNCH="2")
    r = subprocess.run([sys.executable, "-c", RENDERER_CHILD, ROOT, out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    got = np.load(out)
    cnt = dict(zip([str(n) for n in got["names"]], [int(v) for v in got["counters"]]))
    want_hist, want_cnt, want_skipped, want_states = definition(ref, oracle, 300, 200, CANVASES["zoom"][2], 181, 1337,
                                                                samples=250)
    assert int(got["kernel"]) == PRODUCT
    assert_same((got["hist"], cnt), (want_hist, want_cnt))
    assert cnt["skipped_steps"] == want_skipped
    assert np.array_equal(got["states"].view(np.uint32), want_states)


def test_two_renderers_and_the_reduce_after_anti_passes(cb, ref, oracle):
    """Two ranks rehearsed on one device: subsequences [0, t) and [t, 2 t), then cb_renderers_reduce."""
    w, h, box, m, t, passes = 300, 200, CANVASES["zoom"][2], 181, 4096, 2
    dims = cb.FractalDimensions.make(w, h, *box)
    shards = [cb.Renderer(dims, cb.IterationControl(m, 20), first_subsequence=k * t, n_threads=t) for k in range(2)]
    try:
        for r in shards:
            r.render_passes(passes, cb.CB_KERNEL_DEFAULT | cb.CB_KERNEL_FLAG_ANTI)
            assert cb.lib.cb_debug_last_draw_kernel() == PRODUCT
        second = shards[1].read_histogram()
        cb.renderers_reduce(shards)
        got = shards[0].read_histogram()
        untouched = shards[1].read_histogram()
        counters = [r.read_counters().as_dict() for r in shards]
    finally:
        for r in shards:
            r.close()
    args = dict(box=box, mode=anti.NAIVE, omp_threads=omp_threads())
    first_hist, first_cnt = anti.render(ref, w, h, m, t, passes, first_subsequence=0, **args)
    second_hist, second_cnt = anti.render(ref, w, h, m, t, passes, first_subsequence=t, **args)
    whole, _ = anti.render(ref, w, h, m, 2 * t, passes, **args)
    assert np.array_equal(first_hist + second_hist, whole)  # the two ranges are the one run of 2 t threads
    assert np.array_equal(second, second_hist) and np.array_equal(untouched, second_hist)
    assert np.array_equal(got, whole)
    assert_same((None, counters[0]), (None, first_cnt))
    assert_same((None, counters[1]), (None, second_cnt))


def test_binary_anti_on_two_ranks_equals_one_run_of_2t_threads(ref, tmp_path):
    """--anti --gpus 2, both ranks on device 0 (CUDABROT_AMD_FAKE_GPUS): rank r renders subsequences [r T, (r + 1) T)."""
    exe = os.path.join(ROOT, "cudabrot")
    assert os.access(exe, os.X_OK), "./cudabrot is not built"
    buf = str(tmp_path / "anti2.bin")
    env = dict(os.environ, CUDABROT_AMD_FAKE_GPUS="1")
    r = subprocess.run([exe, "--anti", "--gpus", "2", "--passes", "2", "--stats", "-w", "300", "-h", "200", "-m", "181",
                        "-o", os.devnull, "-s", buf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^4 Buddhabrot passes took", r.stdout, re.M)  # 2 ranks x 2 passes
    want, cnt = anti.render(ref, 300, 200, 181, 2 * T, 2, mode=anti.NAIVE, omp_threads=omp_threads())
    assert np.array_equal(read_state_file(buf, 200, 300), want)
    stats = json.loads(r.stderr.strip().splitlines()[-1])
    assert stats["status"] == 0
    for k in ("samples", "increments"):
        assert stats[k] == cnt[k], k
