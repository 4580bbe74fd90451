"""Loader of the Phoenix render's CPU restatement (tests/phoenix_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator it uses, as tests/plot_reference.py does it; nothing is built into the tree.  OpenMP is used where the compiler
has it."""

import ctypes as C
import os
import subprocess

import numpy as np

import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = plot.ORACLE
COUNTER_NAMES = plot.COUNTER_NAMES
EXTRA_NAMES = ("skipped_state", "skipped_z_only", "cycles_state", "cycles_z_only")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES + EXTRA_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles phoenix_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libphoenix_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-o", so, os.path.join(HERE, "phoenix_reference.c"), binding.LIB_PATH, "-Wl,-rpath," + ORACLE,
            "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    f64_p = C.POINTER(f64)
    lib.phoenix_draw.argtypes = [C.POINTER(binding.Dims), vp, C.POINTER(binding.Iters), vp, vp, vp, vp, u64, i32,
                                 C.POINTER(Counters), i32]
    lib.phoenix_draw.restype = None
    lib.phoenix_step.argtypes = [f64, f64, f64, f64, f64_p, f64_p, f64_p, f64_p]
    lib.phoenix_step.restype = f64
    return lib


def step(lib, cr, ci, p_re, p_im, r, i, y_re, y_im):
    """One step of the state (z, y) = ((r, i), (y_re, y_im)) under c and p -> (r', i', y_re', y_im', |z'|^2)."""
    v = [C.c_double(x) for x in (r, i, y_re, y_im)]
    m = lib.phoenix_step(cr, ci, p_re, p_im, *[C.byref(x) for x in v])
    return tuple(float(x.value) for x in v) + (float(m),)


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, *, p, projection=plot.IDENTITY, c=None,
         box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None, extra=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], counters dict).
    p: (p_re, p_im); c None: c is sampled, else the fixed c.  Given `states` are advanced in place, a given `hist` is added
    to; a given dict `extra` receives the two discounts skipped_state and skipped_z_only and the samples each rule found,
    cycles_state and cycles_z_only."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w), dtype=np.uint64)
    m = plot.matrix(projection)
    pp = np.array([float(p[0]), float(p[1])], dtype=np.float64)
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = Counters()
    for samples in launches:
        lib.phoenix_draw(C.byref(d), hist.ctypes.data, C.byref(it), m.ctypes.data, None if cc is None else cc.ctypes.data,
                         pp.ctypes.data, st.ctypes.data, n_threads, samples, C.byref(cnt), omp_threads)
    if extra is not None:
        for n in EXTRA_NAMES:
            extra[n] = int(getattr(cnt, n))
    return hist, cnt.as_dict()
