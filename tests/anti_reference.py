"""Loader of the anti-Buddhabrot's CPU restatement (tests/anti_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator it uses; nothing is built into the tree."""

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments", "skipped_steps")
CENSUS_NAMES = ("cycles", "at_m", "rem_zero", "rem_nonzero", "min_q", "max_p")
NAIVE, COMPRESSED = 0, 1
# The M at which the compression decides something: a round of draw_anti_kernel is 12 steps, a chunk 60; a point is first
# saved at 60 and first matched at 120, so at 120, 180 and 240 cycles are found AT k == M and at one more one step before
# the end; M % 60 != 0 gives the weight split q + 1 / q a remainder; M <= 0 is the kernels' early path.
EDGE_M = [-3, 0, 1, 2, 11, 12, 13, 59, 60, 61, 119, 120, 121, 179, 180, 181, 240, 241, 360, 500, 1000]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


class Census(C.Structure):
    """anti_census: what the compressed mode decided (min_q and max_p are 0 while cycles == 0)."""

    _fields_ = [(n, C.c_uint64) for n in CENSUS_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in CENSUS_NAMES}


def load(directory):
    """Compiles anti_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libanti_reference.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma", "-fopenmp", "-I", ORACLE,
                           "-o", so, os.path.join(HERE, "anti_reference.c"), binding.LIB_PATH,
                           "-Wl,-rpath," + ORACLE, "-lm"])
    lib = C.CDLL(so)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    lib.anti_draw.argtypes = [C.POINTER(binding.Dims), vp, i32, i32, i32, vp, u64, i32, C.POINTER(Counters), i32,
                              C.POINTER(Census)]
    lib.anti_points.argtypes = [C.POINTER(binding.Dims), vp, i32, i32, i32, vp, vp, u64, C.POINTER(Counters),
                                C.POINTER(Census)]
    return lib


def render(lib, w, h, max_iter, n_threads, passes, box=(-2.0, 2.0, -2.0, 2.0), ship=False, mode=COMPRESSED,
           omp_threads=0, seed=1337, first_subsequence=0, samples_per_thread=50, states=None, census=False):
    """`passes` launches of n_threads threads x samples_per_thread samples -> (u64 hist [h, w], counters dict), with
    census=True -> (hist, counters dict, census dict).  omp_threads = 0: sequential.  Given `states` are advanced in
    place."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    hist = np.zeros((h, w), dtype=np.uint64)
    cnt, cen = Counters(), Census()
    for _ in range(passes):
        lib.anti_draw(C.byref(d), hist.ctypes.data, max_iter, 1 if ship else 0, mode, st.ctypes.data, n_threads,
                      samples_per_thread, C.byref(cnt), omp_threads, C.byref(cen))
    return (hist, cnt.as_dict(), cen.as_dict()) if census else (hist, cnt.as_dict())


def points(lib, w, h, max_iter, re, im, box=(-2.0, 2.0, -2.0, 2.0), ship=False, mode=COMPRESSED, census=False):
    """Given starting points, one after another -> (u64 hist [h, w], counters dict), with census=True -> (hist,
    counters dict, census dict)."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    re = np.ascontiguousarray(re, dtype=np.float64)
    im = np.ascontiguousarray(im, dtype=np.float64)
    hist = np.zeros((h, w), dtype=np.uint64)
    cnt, cen = Counters(), Census()
    lib.anti_points(C.byref(d), hist.ctypes.data, max_iter, 1 if ship else 0, mode, re.ctypes.data, im.ctypes.data,
                    re.size, C.byref(cnt), C.byref(cen))
    return (hist, cnt.as_dict(), cen.as_dict()) if census else (hist, cnt.as_dict())
