"""Loader of the plotted renders' CPU restatement (tests/plot_reference.c) -- test infrastructure only.

The C file is compiled into a directory the caller gives (a pytest tmp_path) and linked against oracle/liboracle.so, whose
generator and shortcuts it uses; nothing is built into the tree.  OpenMP is used where the compiler has it."""

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

# the names of the command line and the header's codes; PLAIN and SHIP name the two steps without a formula, the
# reference's and its Burning Ship variant, where a formula code is expected (`step` alone takes SHIP)
NAMES = {"tricorn": 1, "celtic": 2, "buffalo": 3, "perpendicular": 4, "celtic-tricorn": 5}
PLAIN, SHIP = 0, -1


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


def matrix(projection):
    p = np.ascontiguousarray(np.asarray(projection, dtype=np.float64).reshape(-1))
    assert p.size == 8
    return p


def demo_table(n):
    """R = k & 255, G = (k * 7) & 255, B = k >> 1 (below 256): neighbours differ, so an off-by-one in k shows."""
    k = np.arange(n, dtype=np.uint32)
    return (k & 255) | (((k * 7) & 255) << 8) | (((k >> 1) & 255) << 16)


def row_of(row):
    """A depth row from an axis name (zr, zi, cr, ci) or four numbers."""
    if isinstance(row, str):
        out = np.zeros(4)
        out[AXES[row]] = 1.0
        return out
    out = np.ascontiguousarray(np.asarray(row, dtype=np.float64).reshape(-1))
    assert out.size == 4
    return out


def window_table(n, windows):
    """Plane j has weight 1 on [lo_j, hi_j), 0 elsewhere: windows = [(lo, hi)] * 3."""
    k = np.arange(n, dtype=np.uint32)
    lut = np.zeros(n, dtype=np.uint32)
    for j, (lo, hi) in enumerate(windows):
        lut |= ((k >= lo) & (k < hi)).astype(np.uint32) << np.uint32(8 * j)
    return lut


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES + ("zero_entry_steps", "chunk_repeats")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


def load(directory):
    """Compiles plot_reference.c into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libplot_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-o", so, os.path.join(HERE, "plot_reference.c"), binding.LIB_PATH, "-Wl,-rpath," + ORACLE,
            "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u64, f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    dims_p, it_p, cnt_p = C.POINTER(binding.Dims), C.POINTER(binding.Iters), C.POINTER(Counters)
    lib.plot_draw.argtypes = [dims_p, vp, it_p, i32, i32, i32, i32, vp, vp, vp, vp, f64, f64, i32, vp, u64, i32, cnt_p, i32]
    lib.plot_draw.restype = None
    lib.plot_step.argtypes = [i32, i32, i32, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    lib.plot_step.restype = f64
    lib.plot_point.argtypes = [vp, f64, f64, f64, f64, C.POINTER(f64), C.POINTER(f64)]
    lib.plot_point.restype = None
    lib.plot_depth.argtypes = [vp, f64, f64, f64, f64]
    lib.plot_depth.restype = f64
    lib.plot_slice.argtypes = [f64, f64, f64, i32]
    lib.plot_slice.restype = i32
    lib.plot_weight.argtypes = [C.c_uint32, i32]
    lib.plot_weight.restype = u64
    lib.plot_slice_entry.argtypes = [f64, f64, f64, i32, vp]
    lib.plot_slice_entry.restype = C.c_int64
    return lib


def code_of(formula):
    """A formula's code from its code or its name."""
    return NAMES[formula] if isinstance(formula, str) else int(formula)


def step(lib, cr, ci, r, i, degree=2, ship=False, formula=PLAIN):
    """One step from z = (r, i) under c = (cr, ci) -> (r', i', |z'|^2).  formula: a code, a name, PLAIN, or SHIP for
    ship=True."""
    f = code_of(formula)
    zr, zi = C.c_double(r), C.c_double(i)
    m = lib.plot_step(max(f, 0), degree, 1 if ship or f == SHIP else 0, cr, ci, C.byref(zr), C.byref(zi))
    return float(zr.value), float(zi.value), float(m)


def point(lib, projection, zr, zi, cr, ci):
    """(u, v) of one point under the projection."""
    p = matrix(projection)
    u, v = C.c_double(), C.c_double()
    lib.plot_point(p.ctypes.data, zr, zi, cr, ci, C.byref(u), C.byref(v))
    return float(u.value), float(v.value)


def depth_of(lib, row, zr, zi, cr, ci):
    """The depth of one point under the row."""
    d = row_of(row)
    return float(lib.plot_depth(d.ctypes.data, zr, zi, cr, ci))


def slice_of(lib, d, lo, hi, slices):
    """The slice of the depth d in the window [lo, hi) cut into `slices`; None outside."""
    s = int(lib.plot_slice(float(d), float(lo), float(hi), int(slices)))
    return None if s < 0 else s


def entry_of(lib, d, lo, hi, lut):
    """The entry of the depth d in the window [lo, hi) cut into len(lut) slices; None outside."""
    table = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    e = int(lib.plot_slice_entry(float(d), float(lo), float(hi), int(table.size), table.ctypes.data))
    return None if e < 0 else e


def weights(lut):
    """[n, 3] u64: weight_j of every entry of a table."""
    t = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
    return np.stack([(t >> np.uint32(8 * j)) & np.uint32(0xFF) for j in range(3)], axis=1).astype(np.uint64)


def combine(lut, planes):
    """Consequence 1 of "Depth-palette render": [3, h, w], plane j = sum over s of weight_j(lut[s]) * planes[s], in
    uint64."""
    w = weights(lut)
    assert w.shape[0] == planes.shape[0]
    out = np.zeros((3,) + planes.shape[1:], dtype=np.uint64)
    for s in range(planes.shape[0]):
        for j in range(3):
            if w[s, j]:
                out[j] += w[s, j] * planes[s]
    return out


def draw(lib, w, h, max_iter, min_iter, n_threads, launches, *, projection=IDENTITY, degree=2, ship=False, formula=0,
         c=None, lut=None, depth=None, reject=None, box=(-2.0, 2.0, -2.0, 2.0), omp_threads=0, seed=1337,
         first_subsequence=0, states=None, hist=None, extra=None):
    """One launch per entry of `launches` (samples per thread) on the same generators -> (u64 hist, counters dict).
    formula: a code or a name, 0 for none; c None: c is sampled, else the fixed c of a Julia render.  The sink: hist is
    [h, w]; with lut, a table of max_iter entries by escape index, [3, h, w]; with depth = (row, min, max, slices),
    [slices, h, w]; with depth and lut, a table of `slices` entries by slice, [3, h, w] -- a table by escape index under a
    depth is not defined.  reject: whether samples in the cardioid or the bulb are dropped unseen; None is the
    product's rule -- exactly when c is sampled under the reference's own step (no formula, degree 2, no ship).  Given
    `states` are advanced in place, a given `hist` is added to; a given dict `extra` receives zero_entry_steps (the replay
    steps of the accepted orbits whose entry has no weight) and chunk_repeats (the samples that met a bit-identical earlier
    point at a multiple of 60 steps below max_iter)."""
    from oracle import binding

    f = code_of(formula)
    if reject is None:
        reject = c is None and f == 0 and degree == 2 and not ship
    d = binding.make_dims(w, h, *box)
    it = binding.Iters(max_iter, min_iter)
    st = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    row, lo, hi, slices = (None, 0.0, 0.0, 0) if depth is None else depth
    dr = None if depth is None else row_of(row)
    if hist is None:
        hist = np.zeros((3, h, w) if lut is not None else (h, w) if depth is None else (slices, h, w), dtype=np.uint64)
    p = matrix(projection)
    table = None
    if lut is not None:
        table = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
        assert table.size == (max_iter if depth is None else slices)  # by escape index, or by slice: never both
    cc = None if c is None else np.array([float(c[0]), float(c[1])], dtype=np.float64)
    cnt = Counters()
    for samples in launches:
        lib.plot_draw(C.byref(d), hist.ctypes.data, C.byref(it), f, degree, 1 if ship else 0, 1 if reject else 0,
                      p.ctypes.data, None if cc is None else cc.ctypes.data, None if table is None else table.ctypes.data,
                      None if dr is None else dr.ctypes.data, float(lo), float(hi), int(slices), st.ctypes.data, n_threads,
                      samples, C.byref(cnt), omp_threads)
    if extra is not None:
        extra["zero_entry_steps"] = int(cnt.zero_entry_steps)
        extra["chunk_repeats"] = int(cnt.chunk_repeats)
    return hist, cnt.as_dict()
