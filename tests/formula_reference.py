"""Loader of the formula render's CPU restatement (tests/formula_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator it uses; nothing is built into the tree.  OpenMP is used where the compiler has it."""

import ctypes as C
import os
import subprocess

import numpy as np

from project_reference import HOLOGRAM, IDENTITY, ZR_CR, matrix  # noqa: F401  (the matrices the formula tests plot on)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")
# the names of the command line and the header's codes; PLAIN and SHIP are formula_step's two extra steps, the
# reference's and its Burning Ship variant, which the identities compare with
NAMES = {"tricorn": 1, "celtic": 2, "buffalo": 3, "perpendicular": 4, "celtic-tricorn": 5}
PLAIN, SHIP = 0, -1


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES + ("zero_entry_steps", "chunk_repeats")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles formula_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libformula_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-o", so, os.path.join(HERE, "formula_reference.c"), binding.LIB_PATH, "-Wl,-rpath," + ORACLE,
            "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.formula_draw.argtypes = [dims_p, vp, it_p, i32, vp, vp, vp, vp, u64, i32, cnt_p, i32]
    lib.formula_draw.restype = None
    lib.formula_step.argtypes = [i32, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    lib.formula_step.restype = f64
    return lib


def step(lib, f, cr, ci, r, i):
    """One step of formula f (a code, PLAIN or SHIP) from z = (r, i) -> (r', i', |z'|^2)."""
    zr, zi = C.c_double(r), C.c_double(i)
    m = lib.formula_step(int(f), cr, ci, C.byref(zr), C.byref(zi))
    return zr.value, zi.value, m


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, formula, c=None, lut=None, projection=IDENTITY,
         box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None, extra=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], or [3, h, w]
    with a table, counters dict).  formula: a code or a name; c None: c is sampled, else the fixed c of a Julia render;
    lut None: one plane.  Given `states` are advanced in place, a given `hist` is added to; a given dict `extra` receives
    zero_entry_steps and chunk_repeats."""
    from oracle import binding

    f = NAMES[formula] if isinstance(formula, str) else int(formula)
    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w) if lut is None else (3, h, w), dtype=np.uint64)
    p = matrix(projection)
    table = None
    if lut is not None:
        table = np.ascontiguousarray(lut, dtype=np.uint32)
        assert table.size == max_iter
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = Counters()
    for samples in launches:
        lib.formula_draw(C.byref(d), hist.ctypes.data, C.byref(it), f, p.ctypes.data,
                         None if cc is None else cc.ctypes.data, None if table is None else table.ctypes.data,
                         st.ctypes.data, n_threads, samples, C.byref(cnt), omp_threads)
    if extra is not None:
        extra["zero_entry_steps"] = int(cnt.zero_entry_steps)
        extra["chunk_repeats"] = int(cnt.chunk_repeats)
    return hist, cnt.as_dict()
