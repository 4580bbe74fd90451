"""Loader of the depth-palette render's CPU restatement (tests/depth_palette_reference.c) -- test infrastructure only.

The C file includes tests/depth_reference.c (and through it tests/plot_reference.c) and is compiled, like them, into a
directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so; nothing is built into the tree.
The loaded library has depth_reference's functions too: depth_reference.draw works on it."""

import ctypes as C
import os
import subprocess

import numpy as np

import depth_reference as depth
import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))


def load(directory):
    """Compiles depth_palette_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libdepth_palette_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", plot.ORACLE, "-I", HERE, "-o", so, os.path.join(HERE, "depth_palette_reference.c"), binding.LIB_PATH,
            "-Wl,-rpath," + plot.ORACLE, "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u32, u64, f64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(plot.Counters)
    lib.depth_palette_draw.argtypes = [dims_p, vp, it_p, i32, i32, i32, i32, vp, vp, vp, f64, f64, i32, vp, vp, u64, i32,
                                       cnt_p, i32]
    lib.depth_palette_draw.restype = None
    lib.depth_palette_weight.argtypes = [u32, i32]
    lib.depth_palette_weight.restype = u64
    lib.depth_palette_entry.argtypes = [f64, f64, f64, i32, vp]
    lib.depth_palette_entry.restype = C.c_int64
    # depth_reference.c's, which this library includes
    lib.depth_draw.argtypes = [dims_p, vp, it_p, i32, i32, i32, i32, vp, vp, vp, f64, f64, i32, vp, u64, i32, cnt_p, i32]
    lib.depth_draw.restype = None
    lib.depth_slice.argtypes = [f64, f64, f64, i32]
    lib.depth_slice.restype = i32
    lib.depth_point.argtypes = [vp, f64, f64, f64, f64]
    lib.depth_point.restype = f64
    return lib


def entry_of(lib, d, lo, hi, lut):
    """The entry of the depth d in the window [lo, hi) cut into len(lut) slices; None outside."""
    table = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    e = int(lib.depth_palette_entry(float(d), float(lo), float(hi), int(table.size), table.ctypes.data))
    return None if e < 0 else e


def weights(lut):
    """[n, 3] u64: weight_j of every entry of a table."""
    t = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    return np.stack([(t >> np.uint32(8 * j)) & np.uint32(0xFF) for j in range(3)], axis=1).astype(np.uint64)


def combine(lut, planes):
    """Consequence 1 of the definition: [3, h, w], plane j = sum over s of weight_j(lut[s]) * planes[s], in uint64."""
    w = weights(lut)
    assert w.shape[0] == planes.shape[0]
    out = np.zeros((3,) + planes.shape[1:], dtype=np.uint64)
    for s in range(planes.shape[0]):
        for j in range(3):
            if w[s, j]:
                out[j] += w[s, j] * planes[s]
    return out


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, depth_block, lut, *, projection=plot.IDENTITY, degree=2,
         ship=False, formula=0, c=None, reject=None, box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337,
         first_subsequence=0, states=None, extra=None):
    """depth_reference.draw with a table: depth_block = (row, min, max, slices), lut `slices` u32 entries -> (u64 hist
    [3, h, w], counters dict).  reject None is the product's rule: exactly when c is sampled under the reference's own
    step.  A given dict `extra` receives chunk_repeats, as there."""
    from oracle import binding

    f = plot.code_of(formula)
    if reject is None:
        reject = c is None and f == 0 and degree == 2 and not ship
    row, lo, hi, slices = depth_block
    table = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    assert table.size == slices
    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    hist = np.zeros((3, h, w), dtype=np.uint64)
    p = plot.matrix(projection)
    dr = depth.row_of(row)
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = plot.Counters()
    for samples in launches:
        lib.depth_palette_draw(C.byref(d), hist.ctypes.data, C.byref(it), f, degree, 1 if ship else 0, 1 if reject else 0,
                               p.ctypes.data, None if cc is None else cc.ctypes.data, dr.ctypes.data, float(lo), float(hi),
                               int(slices), table.ctypes.data, st.ctypes.data, n_threads, samples, C.byref(cnt), omp_threads)
    if extra is not None:
        extra["chunk_repeats"] = int(cnt.chunk_repeats)
    return hist, cnt.as_dict()
