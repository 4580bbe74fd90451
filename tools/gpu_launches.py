"""The one place where a sequence of direct launches is set up and read back -- the scaffolding of tools/gpu_fuzz.py and,
through tests/device_launches.py, of every GPU suite.  Plain Python and numpy, torch imported where a buffer is made, no
pytest.  It lives beside the fuzzer because tests/ runs the tools and never the other way round.

  Launches          the buffers of a run on device 0 (output, generator states, counters, workspace, carry, u32 tables),
                    launches on them through any entry point, and the read-back (hist, counters dict, kernel id, states);
  renderer_render   the same four through cb.Renderer;
  assert_same       the comparison of two such results;
  SAME, SQUARE, counter_names, omp_threads, planar_states, run, gpu_run: what the suites share beside them.

A harness function of a suite says which entry point and which arguments; everything else is here.
"""

import os
import subprocess

import numpy as np

# every counter but skipped_steps, the clocks and status: what product kernel, lock-step kernel and a CPU reference share
SAME = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps", "increments")
SQUARE = (-2.0, 2.0, -2.0, 2.0)


def omp_threads():
    """The OpenMP workers of a CPU reference: what the environment grants this command (never the machine's core count)."""
    v = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    return int(v) if v.isdigit() and int(v) > 0 else 16


def planar_states(states):
    """The oracle's generator states (d, x[5]) as the library's six planes x0 .. x4, d."""
    return np.concatenate([states["x"][:, j] for j in range(5)] + [states["d"]]).astype(np.uint32)


def run(exe, *args, timeout=120, **kw):
    """The binary where it touches no device, or ends at once on a box without one."""
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, **kw)


def gpu_run(exe, *args, **kw):
    """The binary where it renders."""
    return run(exe, *args, timeout=600, **kw)


def counter_names(cb):
    """The members of cb_counters, in its order: the keys of every counters dict here."""
    return [f[0] for f in cb.Counters._fields_]


class Launches:
    """The buffers of one run on device 0 and the launches on them.

    The output is planes x h x w u64 ([h, w] when planes is None), or `words` u32 words (the focus probe's mask), zeroed or
    hist0.  The generators are fresh: seed (1337) and subsequences [first, first + threads).  The counters are
    len(cb.Counters._fields_) words, zeroed or counters0, or with no_counters absent (d_counters = NULL; they read back as
    zeros).  workspace: a byte count to allocate, or (torch buffer, bytes); carry: True for a zeroed buffer, or a torch
    buffer; tables: u32 arrays by name, whose device copies (self.tables[name]) live as long as the run."""

    def __init__(self, cb, dims, threads, *, planes=None, words=None, hist0=None, seed=None, first=0, counters0=None,
                 no_counters=False, workspace=0, carry=None, tables=None):
        import torch

        self.cb, self.torch, self.dims, self.threads, self.planes, self.words = cb, torch, dims, threads, planes, words
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        if hist0 is not None:
            self.out = self.on_device(hist0, np.uint64)
        elif words is not None:
            self.out = torch.zeros(words, dtype=torch.int32, device=self.dev)
        else:
            self.out = torch.zeros((planes or 1) * dims.w * dims.h, dtype=torch.int64, device=self.dev)
        self.names = counter_names(cb)
        if no_counters:
            self.counters = None
        elif counters0 is None:
            self.counters = torch.zeros(len(self.names), dtype=torch.int64, device=self.dev)
        else:
            self.counters = self.on_device(counters0, np.uint64)
            assert self.counters.numel() == len(self.names)
        self.states = torch.empty(cb.rng_state_bytes(threads), dtype=torch.uint8, device=self.dev)
        cb.initialize_rng(cb.CB_DEFAULT_RNG_SEED if seed is None else seed, first, threads, self.states.data_ptr(),
                          self.stream)
        self.ws, self.ws_bytes = workspace if isinstance(workspace, tuple) else (None, int(workspace))
        if self.ws is None and self.ws_bytes:
            self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        self.carry = torch.zeros(cb.carry_bytes(threads), dtype=torch.uint8, device=self.dev) if carry is True else carry
        self.tables = {k: self.on_device(v, np.uint32) for k, v in (tables or {}).items()}
        self.kernel = None

    def on_device(self, array, dtype):
        """A flat device copy of a u32 or u64 array (torch has the signed types only)."""
        signed = {np.uint32: np.int32, np.uint64: np.int64}[dtype]
        return self.torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).reshape(-1).view(signed).copy()).to(self.dev)

    def launch(self, entry, samples, variant=None, *, workspace=True, flush=True, **extra):
        """One launch of entry(dims, output, states, threads, samples, counters, variant, current stream, **extra) ->
        cb_debug_last_draw_kernel after it.  cb.draw_buddhabrot and cb.draw_buddhabrot_channels are given the workspace
        (workspace=False: this launch goes without) and the carry buffer as well, and with a workspace are followed by their
        cb_flush_scatter (flush=False: by nothing -- an anti launch defers nothing)."""
        cb = self.cb
        args = dict(dims=self.dims, d_states=self.states.data_ptr(), n_threads=self.threads, samples_per_thread=samples,
                    d_counters=self.counters.data_ptr() if self.counters is not None else 0,
                    kernel_variant=cb.CB_KERNEL_DEFAULT if variant is None else variant, stream=self.stream, **extra)
        args["d_mask" if entry is cb.focus_probe else "d_hist"] = self.out.data_ptr()
        ws, ws_bytes = (self.ws.data_ptr(), self.ws_bytes) if workspace and self.ws_bytes else (0, 0)
        if entry in (cb.draw_buddhabrot, cb.draw_buddhabrot_channels):
            args.update(d_workspace=ws, workspace_bytes=ws_bytes, d_carry=self.carry.data_ptr() if self.carry is not None else 0)
        entry(**args)
        self.kernel = cb.lib.cb_debug_last_draw_kernel()
        if ws_bytes and flush and entry is cb.draw_buddhabrot:
            cb.flush_scatter(self.dims, self.out.data_ptr(), self.threads, ws, ws_bytes, self.stream)
        elif ws_bytes and flush and entry is cb.draw_buddhabrot_channels:
            cb.flush_scatter_channels(self.dims, self.out.data_ptr(), len(extra["windows"]), self.threads, ws, ws_bytes,
                                      self.stream)
        return self.kernel

    def launches(self, entry, samples, variant=None, *, drain=None, **extra):
        """One launch per entry of `samples` (samples per thread), one after another on the same buffers.  drain: "launch"
        ends with a launch of 0 samples, "flag" sets CB_KERNEL_FLAG_DRAIN on the last launch.  -> self"""
        variant = self.cb.CB_KERNEL_DEFAULT if variant is None else variant
        samples = list(samples)
        for i, s in enumerate(samples):
            last = drain == "flag" and i + 1 == len(samples)
            self.launch(entry, s, variant | (self.cb.CB_KERNEL_FLAG_DRAIN if last else 0), **extra)
        if drain == "launch":
            self.launch(entry, 0, variant, **extra)
        return self

    def read_counters(self):
        """Synchronises -> the counters as a dict keyed by cb.Counters._fields_."""
        self.torch.cuda.synchronize()
        v = np.zeros(len(self.names), np.uint64) if self.counters is None else self.counters.cpu().numpy().view(np.uint64)
        return {n: int(v[k]) for k, n in enumerate(self.names)}

    def read(self, on_device=False):
        """Synchronises -> (hist, counters dict, cb_debug_last_draw_kernel after the last launch, generator states as u32
        planes).  hist: u64 [h, w] or [planes, h, w], or the probe's u32 mask words; on_device: the flat torch buffer."""
        cnt = self.read_counters()
        if on_device:
            hist = self.out
        elif self.words is not None:
            hist = self.out.cpu().numpy().view(np.uint32)
        else:
            shape = (self.dims.h, self.dims.w) if self.planes is None else (self.planes, self.dims.h, self.dims.w)
            hist = self.out.cpu().numpy().view(np.uint64).reshape(shape)
        return hist, cnt, self.kernel, self.states.cpu().numpy().view(np.uint32)


def renderer_render(cb, w, h, max_iter, min_iter, threads, passes=None, *, split=None, box=SQUARE, variant=None, first=0,
                    fused=True):
    """cb.Renderer over subsequences [first, first + threads): `passes` in one call (fused=False: one call per pass) or one
    call per entry of `split` -> (hist, counters dict, cb_debug_last_draw_kernel, cb_debug_interior_map_level)."""
    variant = cb.CB_KERNEL_DEFAULT if variant is None else variant
    dims = cb.FractalDimensions.make(w, h, *box)
    with cb.Renderer(dims, cb.IterationControl(max_iter, min_iter), first_subsequence=first, n_threads=threads) as r:
        for p in split or ([passes] if fused else [1] * passes):
            r.render_passes(p, variant)
        hist = r.read_histogram()
        cnt = r.read_counters().as_dict()
    return hist, cnt, cb.lib.cb_debug_last_draw_kernel(), cb.lib.cb_debug_interior_map_level()


def assert_same(got, want, keys=SAME, what=""):
    """got, want: (hist, counters, ...) of the GPU and of what it is held to (a CPU reference, or the GPU again); a None in
    either place is not compared.  No status bit on the GPU's side (nor on the other where it has one), every pixel, and the
    counters of `keys`."""
    (gh, gc), (wh, wc) = got[:2], want[:2]
    if gc is not None and wc is not None:
        assert gc["status"] == 0, "%s: the kernel reported an internal invariant violation: %r" % (what, gc)
        assert wc.get("status", 0) == 0, (what, wc)
    if gh is not None and wh is not None:
        assert gh.shape == wh.shape, (what, gh.shape, wh.shape)
        if not np.array_equal(gh, wh):
            diff = np.argwhere(gh != wh)
            first = tuple(diff[0])
            raise AssertionError("%s: histograms differ at %d pixels, first %r: got %d, want %d" % (
                what, len(diff), first, gh[first], wh[first]))
    if gc is not None and wc is not None:
        for k in keys:
            assert gc[k] == wc[k], "%s: counter %s: got %d, want %d" % (what, k, gc[k], wc[k])
