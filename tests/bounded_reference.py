"""Loader of the bounded render's CPU restatement (tests/bounded_reference.c) -- test infrastructure only.

The C file (which includes tests/plot_reference.c for the steps, the projection and the binning) is compiled into a
directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose generator it uses; nothing is
built into the tree.  OpenMP is used where the compiler has it."""

import ctypes as C
import os
import subprocess

import numpy as np

import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = plot.ORACLE

COUNTER_NAMES = plot.COUNTER_NAMES + ("skipped_steps",)
EXTRA_NAMES = ("escaped", "cycles", "no_cycle", "both_weights", "at_m", "rem_zero", "in_canvas", "off_canvas")
NAIVE, COMPRESSED = 0, 1


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]


class Extra(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in EXTRA_NAMES]


def load(directory):
    """Compiles bounded_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libbounded_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-I", HERE, "-o", so, os.path.join(HERE, "bounded_reference.c"), binding.LIB_PATH,
            "-Wl,-rpath," + ORACLE, "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    lib.bounded_draw.argtypes = [C.POINTER(binding.Dims), vp, i32, i32, i32, i32, vp, vp, i32, vp, u64, i32,
                                 C.POINTER(Counters), C.POINTER(Extra), i32]
    lib.bounded_draw.restype = None
    return lib


def draw(lib, w, h, max_iter, n_threads, launches, *, projection=plot.IDENTITY, degree=2, ship=False, formula=0, c=None,
         box=(-2.0, 2.0, -2.0, 2.0), mode=NAIVE, omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None,
         extra=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], counters dict
    with skipped_steps).  formula: a code or a name, 0 for none; c None: c is sampled, else the fixed c.  mode NAIVE: every
    point with weight 1 (skipped_steps 0); COMPRESSED: the transient and one weighted period.  Given `states` are advanced
    in place, a given `hist` is added to; a given dict `extra` receives EXTRA_NAMES."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w), dtype=np.uint64)
    p = plot.matrix(projection)
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt, ex = Counters(), Extra()
    for samples in launches:
        lib.bounded_draw(C.byref(d), hist.ctypes.data, max_iter, plot.code_of(formula), degree, 1 if ship else 0,
                         p.ctypes.data, None if cc is None else cc.ctypes.data, mode, st.ctypes.data, n_threads, samples,
                         C.byref(cnt), C.byref(ex), omp_threads)
    if extra is not None:
        extra.update({n: int(getattr(ex, n)) for n in EXTRA_NAMES})
    return hist, {n: int(getattr(cnt, n)) for n in COUNTER_NAMES}
