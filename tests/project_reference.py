"""Loader of the projected render's CPU restatement (tests/project_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator and shortcuts it uses; nothing is built into the tree."""

import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")
AXES = {"zr": 0, "zi": 1, "cr": 2, "ci": 3}

IDENTITY = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0))
C_PLANE = ((0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
ZR_CR = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))


def plane(x, y):
    """Unit rows: u = axis x, v = axis y."""
    p = np.zeros((2, 4))
    p[0, AXES[x]] = 1.0
    p[1, AXES[y]] = 1.0
    return p


def rotate(p, x, y, degrees):
    """Both rows of p rotated in the (x, y) coordinate plane, by the host's cos / sin: what `--rotate X,Y:DEG` does for
    an angle that is no multiple of 90."""
    p = np.array(p, dtype=np.float64).reshape(2, 4)
    a, b = AXES[x], AXES[y]
    co, si = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    out = p.copy()
    out[:, a] = p[:, a] * co - p[:, b] * si
    out[:, b] = p[:, a] * si + p[:, b] * co
    return out


# a two-angle rotation with irrational entries: the default plane turned towards (c_re, c_im)
HOLOGRAM = rotate(rotate(IDENTITY, "zr", "cr", 30.0), "zi", "ci", 50.0)


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles project_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libproject_reference.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma", "-fopenmp", "-I", ORACLE,
                           "-o", so, os.path.join(HERE, "project_reference.c"), binding.LIB_PATH,
                           "-Wl,-rpath," + ORACLE, "-lm"])
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.project_draw.argtypes = [dims_p, vp, it_p, i32, vp, vp, u64, i32, cnt_p, i32]
    lib.project_point.argtypes = [vp, f64, f64, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    return lib


def matrix(projection):
    p = np.ascontiguousarray(np.asarray(projection, dtype=np.float64).reshape(-1))
    assert p.size == 8
    return p


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, projection, box=(-2.0, 2.0, -2.0, 2.0), ship=False,
         omp_threads=0, seed=1337, first_subsequence=0, states=None, hist=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist [h, w], counters
    dict).  Given `states` are advanced in place, a given `hist` is added to."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    if hist is None:
        hist = np.zeros((h, w), dtype=np.uint64)
    p = matrix(projection)
    cnt = Counters()
    for samples in launches:
        lib.project_draw(C.byref(d), hist.ctypes.data, C.byref(it), 1 if ship else 0, p.ctypes.data, st.ctypes.data,
                         n_threads, samples, C.byref(cnt), omp_threads)
    return hist, cnt.as_dict()


def point(lib, projection, zr, zi, cr, ci):
    """(u, v) of one point under the projection."""
    p = matrix(projection)
    u, v = C.c_double(), C.c_double()
    lib.project_point(p.ctypes.data, zr, zi, cr, ci, C.byref(u), C.byref(v))
    return float(u.value), float(v.value)
