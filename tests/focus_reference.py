"""Loader of the focused render's CPU restatement (tests/focus_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator and shortcuts it uses; nothing is built into the tree."""

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")

COUNTER_NAMES = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps",
                 "increments")
# The crop boxes of the feature's issue (min_real, max_real, min_imag, max_imag): the seahorse side of the main body, the
# upper right of the cardioid, the needle's tip.
BOXES = {
    "body": (-0.2, 0.0, -0.9, -0.7),
    "elephant": (0.25, 0.45, 0.3, 0.5),
    "needle": (-1.8, -1.7, -0.05, 0.05),
}


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles focus_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libfocus_reference.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma", "-fopenmp", "-I", ORACLE,
                           "-o", so, os.path.join(HERE, "focus_reference.c"), binding.LIB_PATH,
                           "-Wl,-rpath," + ORACLE, "-lm"])
    lib = C.CDLL(so)
    vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.focus_probe.argtypes = [dims_p, it_p, i32, vp, u64, i32, i32, vp, cnt_p, i32]
    lib.focus_draw.argtypes = [dims_p, vp, it_p, i32, vp, u64, i32, i32, vp, u32, cnt_p, i32]
    lib.focus_cells.restype = u32
    lib.focus_cells.argtypes = [i32, vp, i32, vp]
    lib.focus_map.argtypes = [i32, vp, u32, u32, u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(C.c_double),
                              C.POINTER(C.c_double)]
    return lib


def mask_words(level):
    n = 4 << level
    return n * n // 32


def probe(lib, w, h, max_iter, min_iter, n_threads, launches, level, box, ship=False, omp_threads=0, seed=1337,
          first_subsequence=0, states=None):
    """The probe: one launch per entry of `launches` (samples per thread) on the same generators -> (mask u32 words,
    counters dict).  Given `states` are advanced in place."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    mask = np.zeros(mask_words(level), dtype=np.uint32)
    cnt = Counters()
    for samples in launches:
        lib.focus_probe(C.byref(d), C.byref(it), 1 if ship else 0, st.ctypes.data, n_threads, samples, level,
                        mask.ctypes.data, C.byref(cnt), omp_threads)
    return mask, cnt.as_dict()


def cells(lib, level, mask, dilate=1):
    """The mask dilated by `dilate` cells -> ascending cell indices (u32)."""
    m = np.ascontiguousarray(mask, dtype=np.uint32)
    assert m.size == mask_words(level)
    n = 4 << level
    out = np.empty(n * n, dtype=np.uint32)
    found = lib.focus_cells(level, m.ctypes.data, dilate, out.ctypes.data)
    return out[:found].copy()


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, box=(-2.0, 2.0, -2.0, 2.0), level=0, cell_list=None,
         ship=False, omp_threads=0, seed=1337, first_subsequence=0, states=None):
    """The draw: one launch per entry of `launches` (samples per thread) on the same generators, from `cell_list` of
    `level` (None: the uniform source, a normal render) -> (u64 hist [h, w], counters dict).  Given `states` are advanced
    in place."""
    from oracle import binding

    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    hist = np.zeros((h, w), dtype=np.uint64)
    cnt = Counters()
    if cell_list is None:
        ptr, n_cells = None, 0
    else:
        cell_list = np.ascontiguousarray(cell_list, dtype=np.uint32)
        ptr, n_cells = cell_list.ctypes.data, cell_list.size
        assert n_cells > 0
    for samples in launches:
        lib.focus_draw(C.byref(d), hist.ctypes.data, C.byref(it), 1 if ship else 0, st.ctypes.data, n_threads, samples,
                       level, ptr, n_cells, C.byref(cnt), omp_threads)
    return hist, cnt.as_dict()


def mapping(lib, level, cell_list, a, b, x1, x2, y1, y2):
    """The six-draw mapping on given generator outputs -> (j, re, im)."""
    cell_list = np.ascontiguousarray(cell_list, dtype=np.uint32)
    j, re, im = C.c_uint32(), C.c_double(), C.c_double()
    lib.focus_map(level, cell_list.ctypes.data, cell_list.size, a, b, x1, x2, y1, y2, C.byref(j), C.byref(re),
                  C.byref(im))
    return int(j.value), float(re.value), float(im.value)
