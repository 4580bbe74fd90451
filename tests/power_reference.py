"""Loader of the Multibrot render's CPU restatement (tests/power_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator it uses; nothing is built into the tree."""

import ctypes as C
import os
import subprocess

import numpy as np

from project_reference import HOLOGRAM, IDENTITY, ZR_CR, matrix  # noqa: F401  (the matrices the power tests plot on)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES] + [("chunk_repeats", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles power_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libpower_reference.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma", "-fopenmp", "-I", ORACLE,
                           "-o", so, os.path.join(HERE, "power_reference.c"), binding.LIB_PATH,
                           "-Wl,-rpath," + ORACLE, "-lm"])
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.power_draw.argtypes = [dims_p, vp, it_p, i32, vp, vp, u64, i32, cnt_p, i32]
    lib.power_step.restype = f64
    lib.power_step.argtypes = [i32, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    return lib


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, degree, projection=IDENTITY, box=(-2.0, 2.0, -2.0, 2.0),
         omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None, repeats=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], counters
    dict).  Given `states` are advanced in place, a given `hist` is added to; a given list `repeats` receives the number
    of samples that met a bit-identical earlier point at a multiple of 60 steps below max_iter."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w), dtype=np.uint64)
    p = matrix(projection)
    cnt = Counters()
    for samples in launches:
        lib.power_draw(C.byref(d), hist.ctypes.data, C.byref(it), degree, p.ctypes.data, st.ctypes.data, n_threads,
                       samples, C.byref(cnt), omp_threads)
    if repeats is not None:
        repeats.append(int(cnt.chunk_repeats))
    return hist, cnt.as_dict()


def step(lib, degree, cr, ci, r, i):
    """One step of the point (r, i) of the sample (cr, ci) -> (r', i', |z'|^2)."""
    zr, zi = C.c_double(r), C.c_double(i)
    m = lib.power_step(degree, cr, ci, C.byref(zr), C.byref(zi))
    return float(zr.value), float(zi.value), float(m)
