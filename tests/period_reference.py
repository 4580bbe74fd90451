"""Loader of the period-palette render's CPU restatement (tests/period_reference.c) -- test infrastructure only.

The C file (which includes tests/bounded_reference.c, and through it tests/plot_reference.c, for the steps, the projection,
the binning and the schedule) is compiled into a directory the caller gives (a pytest tmp_path) and linked against
oracle/liboracle.so, whose generator it uses; nothing is built into the tree.  OpenMP is used where the compiler has it."""

import ctypes as C
import os
import subprocess

import numpy as np

import bounded_reference as bounded
import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = plot.ORACLE

COUNTER_NAMES = bounded.COUNTER_NAMES
# the classes (a) .. (f) of the bounded samples, the search's steps, the escaping samples
EXTRA_NAMES = ("cycle_period", "cycle_none", "tol_period", "tol_none", "rem_zero", "zero_entry", "search_steps", "escaped")
CLASSES = EXTRA_NAMES[:6]
NAIVE, COMPRESSED = bounded.NAIVE, bounded.COMPRESSED
DEFAULT_EPS = 2.0 ** -66
CONSTANT = 0x010101


class Extra(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in EXTRA_NAMES]


def load(directory):
    """Compiles period_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libperiod_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-I", HERE, "-o", so, os.path.join(HERE, "period_reference.c"), binding.LIB_PATH,
            "-Wl,-rpath," + ORACLE, "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    lib.period_draw.argtypes = [C.POINTER(binding.Dims), vp, i32, i32, i32, i32, vp, vp, vp, i32, f64, i32, vp, u64, i32,
                                C.POINTER(bounded.Counters), C.POINTER(Extra), i32]
    lib.period_draw.restype = None
    lib.bounded_draw.argtypes = [C.POINTER(binding.Dims), vp, i32, i32, i32, i32, vp, vp, i32, vp, u64, i32,
                                 C.POINTER(bounded.Counters), C.POINTER(bounded.Extra), i32]
    lib.bounded_draw.restype = None  # the bounded restatement, compiled in: bounded.draw takes this library too
    return lib


def constant_table(n_entries, entry=CONSTANT):
    return np.full(n_entries, entry, dtype=np.uint32)


def one_hot(n_entries, k, entry=1):
    lut = np.zeros(n_entries, dtype=np.uint32)
    lut[k] = entry
    return lut


def gradient_table(n_entries):
    """Three components, every entry with a weight in some plane and neighbours different: plot.demo_table's colours with
    entry 0 (no period) a gray of its own."""
    lut = plot.demo_table(n_entries).astype(np.uint32)
    lut[0] = 0x030201
    return lut


def draw(lib, w, h, max_iter, n_threads, launches, lut, *, eps=DEFAULT_EPS, projection=plot.IDENTITY, degree=2, ship=False,
         formula=0, c=None, box=(-2.0, 2.0, -2.0, 2.0), mode=NAIVE, omp_threads=0, seed=1337, first_subsequence=0,
         states=None, hist=None, extra=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [3, h, w], counters dict
    with skipped_steps).  lut: the table, 2 .. 1024 u32 entries; J = len(lut) - 1.  The rest as bounded_reference.draw."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((3, h, w), dtype=np.uint64)
    p = plot.matrix(projection)
    table = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    assert 2 <= table.size <= 1024
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt, ex = bounded.Counters(), Extra()
    for samples in launches:
        lib.period_draw(C.byref(d), hist.ctypes.data, max_iter, plot.code_of(formula), degree, 1 if ship else 0,
                        p.ctypes.data, None if cc is None else cc.ctypes.data, table.ctypes.data, table.size, float(eps),
                        mode, st.ctypes.data, n_threads, samples, C.byref(cnt), C.byref(ex), omp_threads)
    if extra is not None:
        extra.update({n: int(getattr(ex, n)) for n in EXTRA_NAMES})
    return hist, {n: int(getattr(cnt, n)) for n in COUNTER_NAMES}
