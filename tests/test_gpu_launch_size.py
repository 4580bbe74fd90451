"""The launch shapes the headline and the renderer run, against independent references.

bench.py times launches of PASSES_PER_STEP = 64 reference passes (262144 threads x 3200 samples, two workspaces
pipelined, a carry buffer and a drain launch); cb_renderer -- what ./cudabrot and integrators call -- fuses 128
(kRendererPassesPerLaunch, capi.hip).  Only at these sizes do the pixel stream's word offsets pass 2^31, does a tile's
gather take many slices (the slice table's binary search, r0 = (s - slice_base[t]) * S, slice_regions_for), and does
the 2^32 - 1 entry cap size a wave's segment.  The chain of references:

  1. at full launch size the product equals draw_simple_kernel (CB_KERNEL_SIMPLE, the lock-step kernel: one lane per
     reference thread, the reference's loop, direct atomics, no queues / workspace / carry / interior map), every
     pixel and every counter;
  2. on 2048-subsequence slices of the same launch shape, both the lock-step kernel and the product equal the oracle.

The lock-step kernel runs in launches of at most LOCKSTEP_PASSES passes: its launches are stateless but for the
generator states, so the split is exact, and no launch of it runs for long on a shared device.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bench  # read-only: the workload's constants and dump_outputs
from device_launches import SAME, SQUARE as BOX, Launches, assert_same, omp_threads

pytestmark = pytest.mark.gpu

WIDE, WAVE = 2, 1
LOCKSTEP_PASSES = 8
RENDERER_PASSES = 128   # kRendererPassesPerLaunch (capi.hip)
# the lock-step passes every test of this file asks for, as cumulative sums from the generators' start: one sweep per
# (config, window) serves them all (C3: bench's timed steps [64, 192), the renderer's [0, 256) and [0, 135); C4:
# [0, 128) and [0, 256); C5: [0, 64) and [0, 128) of each window)
CHECKPOINTS = {"C3": (64, 135, 192, 256), "C4": (128, 256), "C5": (64, 128)}


def canvas(cb, name):
    w, h, max_iter, min_iter = bench.CONFIGS[name]
    box = bench.C5_BOX if name == "C5" else BOX
    windows = bench.C5_WINDOWS if name == "C5" else [(max_iter, min_iter)]
    return cb.FractalDimensions.make(w, h, *box), windows


class LockStep:
    """draw_simple_kernel over generator subsequences [first, first + threads) of seed 1337, one (max, min) window,
    into a u64 histogram and counters of its own (device tensors)."""

    def __init__(self, cb, dims, window, threads=bench.THREADS, first=0):
        self.cb, self.it = cb, cb.IterationControl(*window)
        self.seq = Launches(cb, dims, threads, first=first)
        self.hist = self.seq.out
        self.seconds = 0.0

    def run(self, passes):
        t0 = time.perf_counter()
        while passes > 0:
            n = min(passes, LOCKSTEP_PASSES)
            assert self.seq.launch(self.cb.draw_buddhabrot, n * bench.SAMPLES_PER_PASS, self.cb.CB_KERNEL_SIMPLE,
                                   iterations=self.it) == 3
            self.counter_values()  # synchronises: no launch of it queues behind another
            passes -= n
        self.seconds += time.perf_counter() - t0
        return self

    def counter_values(self):
        return self.seq.read_counters()

    def host_histogram(self):
        return self.seq.read()[0]


@pytest.fixture(scope="module")
def lockstep(cb):
    """lockstep(name, plane, a, b) -> (device histogram, counters) of the lock-step kernel over reference passes
    [a, b) of bench's generators (seed 1337, subsequences [0, THREADS)) with window `plane` of config `name`.  Each
    (config, window) is swept once, up to the last of CHECKPOINTS[name], keeping the cumulative state at each; a range
    is the difference of two of them (integers: exact)."""
    import torch

    sweeps = {}

    def passes(name, plane, a, b):
        key = (name, plane)
        if key not in sweeps:
            dims, windows = canvas(cb, name)
            ls = LockStep(cb, dims, windows[plane])
            snaps, done = {0: (None, {k: 0 for k in SAME + ("status",)})}, 0
            for c in CHECKPOINTS[name]:
                ls.run(c - done)
                done = c
                snaps[c] = (ls.hist.clone(), ls.counter_values())
            print("lock-step %s window %s: %d passes in %.1f s, %.1f Msamples/s" % (
                name, windows[plane], done, ls.seconds, done * bench.THREADS * bench.SAMPLES_PER_PASS / ls.seconds / 1e6))
            del ls
            sweeps[key] = snaps
        (ha, ca), (hb, cb_) = sweeps[key][a], sweeps[key][b]
        cnt = {k: cb_[k] - ca[k] for k in SAME}
        cnt["status"] = cb_["status"] | ca["status"]
        return (hb if ha is None else hb - ha), cnt

    yield passes
    sweeps.clear()
    torch.cuda.empty_cache()


def to_host(t, h, w, planes=1):
    a = t.cpu().numpy().view(np.uint64)
    return a.reshape(h, w) if planes == 1 else a.reshape(planes, h, w)


# ---- 1. bench's dump against the lock-step kernel -------------------------------------------------------------------

@pytest.mark.parametrize("name,warmup,steps", [("C3", 1, 2), ("C4", 0, 2), ("C5", 0, 1)])
def test_bench_dump_equals_the_lock_step_kernel(cb, lockstep, repo_root, tmp_path, monkeypatch, name, warmup, steps):
    """bench.py --dump-outputs of `steps` timed 64-pass launches (after `warmup` of them, and the drain that empties the
    carry before the clock) == the lock-step kernel over the same reference passes, file for file.

    Regimes (kEntriesPerSample = 2.5 entries sized per sample; regions of kRegionEntries = 32768 entries; a gather
    slice of S = max(ceil(pairs / target), 512) regions, at most kSliceRegionsDefault = 8192, where pairs = tiles x
    regions and target = 12288, or 6144 with two levels -- scatter.hip slice_regions_for):
      C3: 262144 x 3200 x 2.5 = 2.10e9 entries sized per launch, just under 2^31; 1.40e9 recorded (1.67 per sample):
          ~11 regions in each of the 4096 wave segments, ~45k regions over 1024 tiles in one group, so
          S = ceil(1024 x 45k / 12288) = ~3.8k and every tile is gathered in ~12 slices.
      C4: 24649 tiles in 25 groups, a chunked stream (kChunkWords = 1024, regions of 32 chunks per group):
          2.10e9 words sized, 1.40e9 recorded = ~1.4M chunks, ~45k regions, ~1.8k per group; S = ~7.5k, so a tile
          takes one slice (two for a group of more than S regions).
      C5: three planes sorted as one canvas of 55578 tiles in 55 groups: 1.5 x 2.10e9 = 3.15e9 words sized, 1.14e9
          recorded, ~42k regions, ~0.8k per group: one slice per tile.
    C5's planes come from three lock-step runs (the lock-step kernel takes one window), each from generators
    seeded and advanced alike; of the fused counters only `samples` and the windows' summed `increments` have a
    per-window meaning."""
    import torch

    out = tmp_path / "bench"
    cmd = [sys.executable, os.path.join(repo_root, "bench.py"), "--gpus", "1", "--warmup", str(warmup),
           "--steps", str(steps), "--dump-outputs", str(out)] + (["--config", name] if name != "C3" else [])
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=repo_root)
    assert r.returncode == 0, r.stderr[-3000:]
    print("bench %s: %.1f s" % (name, time.perf_counter() - t0))

    w, h, _, _ = bench.CONFIGS[name]
    _, windows = canvas(cb, name)
    a = warmup * bench.PASSES_PER_STEP
    b = a + steps * bench.PASSES_PER_STEP
    planes = [lockstep(name, p, a, b) for p in range(len(windows))]
    hist = planes[0][0] if len(planes) == 1 else torch.cat([p[0] for p in planes])
    if len(planes) == 1:
        cnt = planes[0][1]
    else:
        cnt = {k: 0 for k in bench.DUMP_COUNTERS}
        cnt["samples"] = planes[0][1]["samples"]
        cnt["increments"] = sum(p[1]["increments"] for p in planes)
    for _, c in planes:
        assert c["status"] == 0 and c["samples"] == bench.THREADS * bench.SAMPLES_PER_PASS * (b - a)
    ref = tmp_path / "lockstep"
    monkeypatch.setattr(bench, "W", w)   # dump_outputs reads the row length from bench's module global
    bench.dump_outputs(str(ref), hist, cnt, torch, np)
    del hist, planes

    files = sorted(os.listdir(out))
    assert files == sorted(os.listdir(ref)) == ["counters.npy", "histogram_row_sums.npy", "histogram_sample.npy"]
    got = {f: np.load(out / f) for f in files}
    want = {f: np.load(ref / f) for f in files}
    for f in ("histogram_sample.npy", "histogram_row_sums.npy"):
        assert np.array_equal(got[f], want[f]), "%s: %s differs from the lock-step kernel's at %d entries" % (
            name, f, int((got[f] != want[f]).sum()))
    keys = bench.DUMP_COUNTERS if name != "C5" else ("samples", "increments")
    for k in keys:
        i = bench.DUMP_COUNTERS.index(k)
        assert got["counters.npy"][i] == want["counters.npy"][i], (name, k, got["counters.npy"][i], want["counters.npy"][i])
    increments = int(got["counters.npy"][bench.DUMP_COUNTERS.index("increments")])
    print("%s: %.3g increments per %d-pass launch" % (name, increments / steps, bench.PASSES_PER_STEP))


# ---- 2. renderer-sized launches against the lock-step kernel --------------------------------------------------------

def render(cb, name, split):
    """cb.Renderer over bench's generators with the default 128 passes per launch.  (The renderer sizes its two
    workspaces for a full launch, but at most free / 4 each (capi.hip, prepare_for_variant): on a crowded device they
    are smaller, the stream regions fill sooner and more of the increments are added directly.)"""
    dims, windows = canvas(cb, name)
    it = windows if len(windows) > 1 else cb.IterationControl(*windows[0])
    with cb.Renderer(dims, it, n_threads=bench.THREADS) as r:
        for p in split:
            r.render_passes(p)
        kernel = cb.lib.cb_debug_last_draw_kernel()
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
    return hist, cnt, kernel


@pytest.mark.parametrize("name,split", [("C3", [256]), ("C3", [128, 7]), ("C4", [256])],
                         ids=["C3_two_launches", "C3_ragged", "C4_two_launches"])
def test_renderer_launches_equal_the_lock_step_kernel(cb, lockstep, name, split):
    """128-pass launches of cb_renderer (the carry handed from launch to launch; [128, 7]: a ragged last launch) ==
    the lock-step kernel over the same passes, every pixel and every counter.

    C3 at 128 passes: 262144 x 6400 x 2.5 = 4.19e9 entries sized (under the 2^32 - 1 cap), 2.81e9 recorded per
    launch: the segments of the upper half of the waves start beyond word 2^31, and the pixel stream's word offsets
    pass it.  ~21 regions per wave segment, ~88k over 1024 tiles: S = ceil(1024 x 88k / 12288) = ~7.3k regions per
    slice (under 8192), ~12 slices per tile.  [128, 7]: the first launch as above, then one of 7 passes.
    C4 at 128 passes: a chunked stream of 4.19e9 words sized, so chunk offsets w * cap + j * kChunkWords (scatter.hip,
    the chunk list) run up to ~4.2e9, just under 2^32; 2.81e9 words recorded per launch, ~89k regions, ~3.6k per
    group of 1024 tiles: S = 8192 (the cap), one slice per tile but in the densest groups."""
    passes = sum(split)
    hist, cnt, kernel = render(cb, name, split)
    assert kernel == WIDE, "the launches were not taken by draw_wide_kernel"
    launches = sum((p + RENDERER_PASSES - 1) // RENDERER_PASSES for p in split)
    print("%s %r: %.3g increments per launch (2^31 = %.3g)" % (name, split, cnt["increments"] / launches, 2.0 ** 31))
    if split == [256]:
        # the regime: a launch's increments -- the words of its pixel stream -- pass 2^31 (both configs: the canvases
        # share the box, and so the samples that escape inside it)
        assert cnt["increments"] / launches > 2 ** 31
    ref, rc = lockstep(name, 0, 0, passes)
    assert_same((None, cnt), (None, rc), what=name)
    assert cnt["samples"] == bench.THREADS * bench.SAMPLES_PER_PASS * passes
    w, h, _, _ = bench.CONFIGS[name]
    assert_same((hist, None), (to_host(ref, h, w), None), what=name)


def test_renderer_fused_c5_launch_equals_the_lock_step_kernel(cb, lockstep):
    """One 128-pass fused launch of C5's three windows on 20000 x 15000 == three lock-step runs.

    1.5 x 262144 x 6400 x 2.5 = 6.3e9 entries would be sized: the 2^32 - 1 cap decides each wave's segment length
    (cap_limit = 0xffffffff / n_waves, scatter.hip make_bin_layout), not the estimate; ~2.3e9 words recorded, so word
    offsets pass 2^31 (~2.3e9 / 32768 = ~70k regions over 55 groups: one slice per tile).  Fused launches are
    draw_wave_kernel's today: cb_draw_buddhabrot_channels launches no other (C5 on the wide kernel is future work)."""
    passes = RENDERER_PASSES
    hist, cnt, kernel = render(cb, "C5", [passes])
    assert kernel == WAVE
    print("C5 fused: %.3g increments in one launch (2^31 = %.3g)" % (cnt["increments"], 2.0 ** 31))
    assert cnt["status"] == 0
    assert cnt["increments"] > 2 ** 31   # the regime: word offsets of the (capped) stream pass 2^31
    assert cnt["samples"] == bench.THREADS * bench.SAMPLES_PER_PASS * passes
    w, h, _, _ = bench.CONFIGS["C5"]
    increments = 0
    for p in range(len(bench.C5_WINDOWS)):
        ref, rc = lockstep("C5", p, 0, passes)
        assert rc["status"] == 0 and rc["samples"] == cnt["samples"]
        increments += rc["increments"]
        assert_same((hist[p], None), (to_host(ref, h, w), None), what="C5 window %r" % (bench.C5_WINDOWS[p],))
        del ref
    assert cnt["increments"] == increments


# ---- 3. slices of the launch shape against the oracle -----------------------------------------------------------------

SLICE_THREADS = 2048
SLICE_FIRSTS = (0, bench.THREADS // 2 - SLICE_THREADS // 2, bench.THREADS - SLICE_THREADS)


@pytest.mark.parametrize("name,plane", [("C3", 0), ("C4", 0), ("C5", 1)], ids=["C3", "C4", "C5_window_8000_1000"])
def test_slices_equal_the_oracle(cb, oracle, name, plane):
    """Three 2048-subsequence slices of the 262144 (the first, the middle, the last), one 64-pass launch each: the
    lock-step kernel and the product (a renderer of 2048 threads from first_subsequence) both == the oracle, every
    pixel and every counter.  The C3 canvas has dyadic pixels, C4's are 4/20000 (the division path); C5's window
    (8000, 1000) on C5_BOX is one plane of the fused render.  (The oracle: 3 x 6.6e6 samples per canvas.)"""
    dims, windows = canvas(cb, name)
    window = windows[plane]
    box = bench.C5_BOX if name == "C5" else BOX
    passes = bench.PASSES_PER_STEP
    for first in SLICE_FIRSTS:
        what = "%s from subsequence %d" % (name, first)
        with cb.Renderer(dims, cb.IterationControl(*window), n_threads=SLICE_THREADS, first_subsequence=first) as r:
            r.render_passes(passes)
            kernel = cb.lib.cb_debug_last_draw_kernel()
            got = r.read_histogram()
            cnt = r.read_counters().as_dict()
        assert kernel == (WAVE if name == "C5" else WIDE), (what, kernel)
        ls = LockStep(cb, dims, window, threads=SLICE_THREADS, first=first).run(passes)
        lhist, lcnt = ls.host_histogram(), ls.counter_values()
        del ls
        t0 = time.perf_counter()
        ref, rc = oracle.render(dims.w, dims.h, window[0], window[1], SLICE_THREADS, passes, box,
                                first_subsequence=first, omp_threads=omp_threads())
        print("oracle %s: %.1f s" % (what, time.perf_counter() - t0))
        rc = dict(rc, status=0)
        assert_same((lhist, lcnt), (ref, rc), what="lock-step " + what)
        del lhist
        assert_same((got, cnt), (ref, rc), what=what)
        del got, ref


# ---- 4. a drained carry buffer handed to the other kernel ------------------------------------------------------------

@pytest.mark.parametrize("first_wide", [True, False], ids=["wide_then_wave", "wave_then_wide"])
def test_a_drained_carry_buffer_is_any_kernels_to_start_from(cb, first_wide):
    """a launch and its drain with one kernel, then, on the same carry buffer, a launch the library gives to
    the other kernel (min_iter 20: draw_wide_kernel takes it; min_iter 1000, beyond the LONG stage's start: it does
    not) and its drain.  The drain leaves nothing carried, so the second kernel has nothing foreign to report
    (CB_STATUS_CARRY_FOREIGN is for orbits in flight: test_gpu_wide.py), and the sequence equals the lock-step kernel's
    over the same samples."""
    w, h, threads, max_iter, samples = 512, 512, 4096, 2000, 8 * bench.SAMPLES_PER_PASS
    dims = cb.FractalDimensions.make(w, h)
    order = [(20, WIDE), (1000, WAVE)] if first_wide else [(1000, WAVE), (20, WIDE)]
    seq = Launches(cb, dims, threads, workspace=cb.scatter_workspace_bytes(dims, threads, samples), carry=True)
    for min_iter, kernel in order:
        it = cb.IterationControl(max_iter, min_iter)
        for n in (samples, 0):                  # the launch, then the drain of what it carried
            assert seq.launch(cb.draw_buddhabrot, n, iterations=it) == kernel, (min_iter, n)
            status = seq.read_counters()["status"]
            assert status == 0, "status %d after the %s of min_iter %d" % (status, "drain" if n == 0 else "launch", min_iter)
    got, cnt = seq.read()[:2]

    ls = LockStep(cb, dims, (max_iter, order[0][0]), threads=threads)
    ls.run(8)
    ls.it = cb.IterationControl(max_iter, order[1][0])
    ls.run(8)
    assert_same((got, cnt), (ls.host_histogram(), ls.counter_values()), what="carry handed over")
