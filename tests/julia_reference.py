"""Loader of the Julia render's CPU restatement (tests/julia_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator it uses; nothing is built into the tree.  OpenMP is used where the compiler has it."""

import ctypes as C
import os
import subprocess

import numpy as np

from project_reference import HOLOGRAM, IDENTITY, ZR_CR, matrix  # noqa: F401  (the matrices the Julia tests plot on)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles julia_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libjulia_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-o", so, os.path.join(HERE, "julia_reference.c"), binding.LIB_PATH, "-Wl,-rpath," + ORACLE,
            "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.julia_draw.argtypes = [dims_p, vp, it_p, i32, i32, vp, vp, vp, u64, i32, cnt_p, i32]
    lib.julia_draw.restype = None
    lib.julia_step.restype = f64
    lib.julia_step.argtypes = [i32, i32, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    return lib


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, c, degree=2, ship=False, projection=IDENTITY,
         box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], counters
    dict).  Given `states` are advanced in place, a given `hist` is added to."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w), dtype=np.uint64)
    p = matrix(projection)
    cc = np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = Counters()
    for samples in launches:
        lib.julia_draw(C.byref(d), hist.ctypes.data, C.byref(it), degree, 1 if ship else 0, p.ctypes.data, cc.ctypes.data,
                       st.ctypes.data, n_threads, samples, C.byref(cnt), omp_threads)
    return hist, cnt.as_dict()


def step(lib, degree, ship, cr, ci, r, i):
    """One step of the point (r, i) under the fixed c = (cr, ci) -> (r', i', |z'|^2)."""
    zr, zi = C.c_double(r), C.c_double(i)
    m = lib.julia_step(degree, 1 if ship else 0, cr, ci, C.byref(zr), C.byref(zi))
    return float(zr.value), float(zi.value), float(m)
