"""Loader of the aimed render's CPU restatement (tests/aim_reference.c) -- test infrastructure only.

The C file (which includes tests/bounded_reference.c and, through it, tests/plot_reference.c for the steps, the projection,
the binning and the save schedule) is compiled into a directory the caller gives (a pytest tmp_path) and linked against
oracle/liboracle.so, whose generator and shortcuts it uses; nothing is built into the tree.  The mask's dilation and the
cell list are tests/focus_reference.c's (lib.focus).  CASES is the issue's table of aimed renders."""

import ctypes as C
import os
import subprocess

import numpy as np

import focus_reference as focus
import plot_reference as plot

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = plot.ORACLE

COUNTER_NAMES = plot.COUNTER_NAMES + ("skipped_steps",)
EXTRA_NAMES = ("marking", "plotted", "cycles", "no_cycle", "both_weights", "in_canvas", "off_canvas")
NAIVE, COMPRESSED = 0, 1
mask_words = focus.mask_words

# The common shape of the aimed suites: 64 x 48, 1000 threads (a ragged last wave and workgroup), seed 1337, level 6,
# dilate 1, M = 500, -c 20, the probe as two launches of 3 + 13 samples per thread, the draw as 3 + 50 + 1.
W, H, MAX, MIN, THREADS, LEVEL, DILATE = 64, 48, 500, 20, 1000, 6, 1
PROBE, DRAW = (3, 13), (3, 50, 1)

ZR_CR = plot.plane("zr", "cr")
CR_CI = plot.plane("cr", "ci")
# name -> what the un-aimed render is and its window (min u, max u, min v, max v), and the model's figures for the common
# shape: cells marked by the probe, cells listed after dilation, and the aimed draw's plotted samples
CASES = {
    "plane_zr_cr": dict(projection=ZR_CR, box=(-1.0, -0.5, -1.5, -1.25), marked=10, listed=82, plotted=22437),
    "bounded_zr_cr": dict(bounded=True, projection=ZR_CR, box=(-2.0, 2.0, -1.5, -1.25), marked=14, listed=62,
                          cycles=18236, no_cycle=23980),
    "bounded_julia": dict(bounded=True, c=(-1.0, 0.0), box=(-0.5, 0.5, -0.5, 0.5), marked=1307, listed=5645, plotted=48506),
    "julia": dict(c=(-0.123, 0.745), box=(0.2, 0.7, 0.2, 0.7), marked=45, listed=364, plotted=9441),
    "power3_rotated": dict(degree=3, projection=plot.rotate(plot.plane("zr", "zi"), "zi", "cr", 45.0),
                           box=(-0.3, 0.3, 0.4, 0.9), marked=63, listed=507, plotted=11681),
    "identity_body": dict(box=focus.BOXES["body"], marked=39, listed=285, plotted=22150),
    "bounded_cr_ci": dict(bounded=True, projection=CR_CI, box=(-0.3, 0.1, 0.5, 0.9), marked=71, listed=334,
                          cycles=22513, no_cycle=27163),
    "bounded_tricorn_zr_cr": dict(bounded=True, formula="tricorn", projection=ZR_CR, box=(-2.0, 2.0, -1.25, -0.75), marked=79,
                                  listed=365, cycles=31137, no_cycle=16891),
    "ship_identity": dict(ship=True, box=(-1.8, -1.7, -0.1, 0.0), marked=7, listed=63, plotted=28949),
    "bounded_ship_zr_cr": dict(bounded=True, ship=True, projection=ZR_CR, box=(-2.0, 2.0, -1.0, -0.5), marked=332,
                               listed=1443, cycles=15513, no_cycle=35293),
    "bounded_julia_130": dict(bounded=True, c=(-0.123, 0.745), max_iter=130, box=(-0.5, 0.5, -0.5, 0.5), marked=1181,
                              listed=5361, cycles=45338, no_cycle=279),
}
MODEL_KEYS = ("marked", "listed", "plotted", "cycles", "no_cycle")


def shape_of(kw):
    """The common shape with a case's (or a test's) own entries over it; the model's figures are dropped."""
    s = dict(w=W, h=H, box=(-2.0, 2.0, -2.0, 2.0), max_iter=MAX, min_iter=MIN, threads=THREADS, level=LEVEL, dilate=DILATE,
             probe=PROBE, draw=DRAW, bounded=False, c=None, projection=plot.IDENTITY, degree=2, ship=False, formula=0)
    s.update({k: v for k, v in kw.items() if k not in MODEL_KEYS})
    return s


def rejects(s):
    """Cardioid and bulb: the Mandelbrot step on a sampled c of the escaping kind."""
    return not s["bounded"] and s["c"] is None and not s["formula"] and s["degree"] == 2 and not s["ship"]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]


class Extra(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in EXTRA_NAMES]


def load(directory):
    """Compiles aim_reference.c (and focus_reference.c, as lib.focus) into `directory` and returns the loaded library."""
    from oracle import binding  # builds liboracle.so if it is missing

    so = os.path.join(str(directory), "libaim_reference.so")
    base = ["gcc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"]
    rest = ["-I", ORACLE, "-I", HERE, "-o", so, os.path.join(HERE, "aim_reference.c"), binding.LIB_PATH,
            "-Wl,-rpath," + ORACLE, "-lm"]
    if subprocess.call(base + ["-fopenmp"] + rest, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + rest)  # a compiler without OpenMP: one thread, the same result
    lib = C.CDLL(so)
    vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    lib.aim_launch.argtypes = [C.POINTER(binding.Dims), vp, vp, C.POINTER(binding.Iters), i32, i32, i32, i32, i32, vp, vp,
                               i32, vp, u64, i32, i32, vp, u32, C.POINTER(Counters), C.POINTER(Extra), i32]
    lib.aim_launch.restype = None
    lib.aim_map.argtypes = [i32, vp, u32, u32, u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(C.c_double),
                            C.POINTER(C.c_double)]
    lib.aim_map.restype = None
    lib.focus = focus.load(directory)
    return lib


def _launches(lib, s, launches, mode, omp_threads, states, hist, mask, cell_list, extra):
    from oracle import binding

    d = binding.make_dims(s["w"], s["h"], *s["box"])
    it = binding.Iters(s["max_iter"], s["min_iter"])
    st = binding.init_states(s.get("seed", 1337), 0, s["threads"]) if states is None else states
    p = plot.matrix(s["projection"])
    cc = None if s["c"] is None else np.array([float(s["c"][0]), float(s["c"][1])], dtype=np.float64)
    if cell_list is None:
        ptr, n_cells, level = None, 0, s["level"] if mask is not None else 0
    else:
        cell_list = np.ascontiguousarray(cell_list, dtype=np.uint32)
        ptr, n_cells, level = cell_list.ctypes.data, cell_list.size, s["level"]
        assert n_cells > 0
    cnt, ex = Counters(), Extra()
    for samples in launches:
        lib.aim_launch(C.byref(d), None if hist is None else hist.ctypes.data, None if mask is None else mask.ctypes.data,
                       C.byref(it), 1 if s["bounded"] else 0, plot.code_of(s["formula"]), s["degree"], 1 if s["ship"] else 0,
                       1 if rejects(s) else 0, p.ctypes.data, None if cc is None else cc.ctypes.data, mode, st.ctypes.data,
                       s["threads"], samples, level, ptr, n_cells, C.byref(cnt), C.byref(ex), omp_threads)
    if extra is not None:
        extra.update({n: int(getattr(ex, n)) for n in EXTRA_NAMES})
    return {n: int(getattr(cnt, n)) for n in COUNTER_NAMES}


def probe(lib, mode=NAIVE, omp_threads=0, states=None, extra=None, **kw):
    """The probe: one launch per entry of shape_of(kw)["probe"] on the same generators -> (mask u32 words, counters dict).
    Given `states` are advanced in place; a given dict `extra` receives EXTRA_NAMES."""
    s = shape_of(kw)
    mask = np.zeros(mask_words(s["level"]), dtype=np.uint32)
    return mask, _launches(lib, s, s["probe"], mode, omp_threads, states, None, mask, None, extra)


def cells(lib, mask, **kw):
    """The mask dilated by shape_of(kw)["dilate"] cells -> ascending cell indices (u32): tests/focus_reference.c's."""
    s = shape_of(kw)
    return focus.cells(lib.focus, s["level"], mask, s["dilate"])


def draw(lib, cell_list, mode=NAIVE, omp_threads=0, states=None, extra=None, **kw):
    """The draw: one launch per entry of shape_of(kw)["draw"] on the same generators, from `cell_list` (None: the uniform
    source, the un-aimed render) -> (u64 hist [h, w], counters dict with skipped_steps)."""
    s = shape_of(kw)
    hist = np.zeros((s["h"], s["w"]), dtype=np.uint64)
    return hist, _launches(lib, s, s["draw"], mode, omp_threads, states, hist, None, cell_list, extra)


def mapping(lib, level, cell_list, a, b, x1, x2, y1, y2):
    """The six-draw mapping on given generator outputs -> (j, re, im)."""
    cell_list = np.ascontiguousarray(cell_list, dtype=np.uint32)
    j, re, im = C.c_uint32(), C.c_double(), C.c_double()
    lib.aim_map(level, cell_list.ctypes.data, cell_list.size, a, b, x1, x2, y1, y2, C.byref(j), C.byref(re), C.byref(im))
    return int(j.value), float(re.value), float(im.value)
