"""Loader of the palette render's CPU restatement (tests/palette_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator and shortcuts it uses; nothing is built into the tree.  OpenMP is used where the compiler has it."""

import ctypes as C
import os
import subprocess

import numpy as np

from project_reference import HOLOGRAM, IDENTITY, ZR_CR, matrix  # noqa: F401  (the matrices the palette tests plot on)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES + ("zero_entry_steps",)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles palette_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libpalette_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-o", so, os.path.join(HERE, "palette_reference.c"), binding.LIB_PATH, "-Wl,-rpath," + ORACLE,
            "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.palette_draw.argtypes = [dims_p, vp, it_p, i32, i32, vp, i32, vp, vp, vp, u64, i32, cnt_p, i32]
    lib.palette_draw.restype = None
    return lib


def demo_table(n):
    """R = k & 255, G = (k * 7) & 255, B = k >> 1 (below 256): neighbours differ, so an off-by-one in k shows."""
    k = np.arange(n, dtype=np.uint32)
    return (k & 255) | (((k * 7) & 255) << 8) | (((k >> 1) & 255) << 16)


def window_table(n, windows):
    """Plane j has weight 1 on [lo_j, hi_j), 0 elsewhere: windows = [(lo, hi)] * 3."""
    k = np.arange(n, dtype=np.uint32)
    lut = np.zeros(n, dtype=np.uint32)
    for j, (lo, hi) in enumerate(windows):
        lut |= ((k >= lo) & (k < hi)).astype(np.uint32) << np.uint32(8 * j)
    return lut


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, lut, c=None, degree=2, ship=False, projection=IDENTITY,
         box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [3, h, w], counters
    dict, replay steps of the accepted orbits whose entry has no weight).  c None: c is sampled; else the fixed c of a
    Julia render.  Given `states` are advanced in place, a given `hist` is added to."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((3, h, w), dtype=np.uint64)
    p = matrix(projection)
    table = np.ascontiguousarray(lut, dtype=np.uint32)
    assert table.size == max_iter
    cc = np.array([0.0, 0.0] if c is None else [float(c[0]), float(c[1])], dtype=np.float64)
    cnt = Counters()
    for samples in launches:
        lib.palette_draw(C.byref(d), hist.ctypes.data, C.byref(it), degree, 1 if ship else 0, p.ctypes.data,
                         0 if c is None else 1, cc.ctypes.data, table.ctypes.data, st.ctypes.data, n_threads, samples,
                         C.byref(cnt), omp_threads)
    return hist, cnt.as_dict(), int(cnt.zero_entry_steps)
