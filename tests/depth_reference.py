"""Loader of the depth render's CPU restatement (tests/depth_reference.c) -- test infrastructure only.

The C file includes tests/plot_reference.c and is compiled, like it, into a directory the caller gives (a pytest tmp_path)
and linked against oracle/liboracle.so; nothing is built into the tree."""

import ctypes as C
import os
import subprocess

import numpy as np

import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))


def row_of(row):
    """A depth row from an axis name (zr, zi, cr, ci) or four numbers."""
    if isinstance(row, str):
        out = np.zeros(4)
        out[plot.AXES[row]] = 1.0
        return out
    out = np.ascontiguousarray(np.asarray(row, dtype=np.float64).reshape(-1))
    assert out.size == 4
    return out


def load(directory):
    """Compiles depth_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libdepth_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", plot.ORACLE, "-I", HERE, "-o", so, os.path.join(HERE, "depth_reference.c"), binding.LIB_PATH,
            "-Wl,-rpath," + plot.ORACLE, "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(plot.Counters)
    lib.depth_draw.argtypes = [dims_p, vp, it_p, i32, i32, i32, i32, vp, vp, vp, f64, f64, i32, vp, u64, i32, cnt_p, i32]
    lib.depth_draw.restype = None
    lib.depth_slice.argtypes = [f64, f64, f64, i32]
    lib.depth_slice.restype = i32
    lib.depth_point.argtypes = [vp, f64, f64, f64, f64]
    lib.depth_point.restype = f64
    return lib


def slice_of(lib, d, lo, hi, slices):
    """The slice of the depth d in the window [lo, hi) cut into `slices`; None outside."""
    s = int(lib.depth_slice(float(d), float(lo), float(hi), int(slices)))
    return None if s < 0 else s


def point(lib, row, zr, zi, cr, ci):
    """The depth of one point under the row."""
    d = row_of(row)
    return float(lib.depth_point(d.ctypes.data, zr, zi, cr, ci))


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, depth, *, projection=plot.IDENTITY, degree=2, ship=False,
         formula=0, c=None, reject=None, box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337, first_subsequence=0,
         states=None, extra=None):
    """plot_reference.draw without a table and with depth = (row, min, max, slices) -> (u64 hist [slices, h, w], counters
    dict).  reject None is the product's rule: exactly when c is sampled under the reference's own step.  A given dict
    `extra` receives chunk_repeats: the samples that met a bit-identical earlier point at a multiple of 60 steps below
    max_iter -- what the product kernel's early-out can retire."""
    from oracle import binding

    f = plot.code_of(formula)
    if reject is None:
        reject = c is None and f == 0 and degree == 2 and not ship
    row, lo, hi, slices = depth
    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    hist = np.zeros((slices, h, w), dtype=np.uint64)
    p = plot.matrix(projection)
    dr = row_of(row)
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = plot.Counters()
    for samples in launches:
        lib.depth_draw(C.byref(d), hist.ctypes.data, C.byref(it), f, degree, 1 if ship else 0, 1 if reject else 0,
                       p.ctypes.data, None if cc is None else cc.ctypes.data, dr.ctypes.data, float(lo), float(hi),
                       int(slices), st.ctypes.data, n_threads, samples, C.byref(cnt), omp_threads)
    if extra is not None:
        extra["chunk_repeats"] = int(cnt.chunk_repeats)
    return hist, cnt.as_dict()
