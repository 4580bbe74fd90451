"""ctypes binding of include/cudabrot_amd.h -- one Python name per C entry point, nothing more.

Names follow the reference's own (cudabrot.cu): FractalDimensions (:46-58), IterationControl (:62-67),
InitializeRNG (:146-149) -> initialize_rng, DrawBuddhabrot (:379-414) -> draw_buddhabrot,
RecomputePixelDeltas (:505-527), SetGrayscalePixels (:454-468), SaveImage (:548-577); Renderer is
SetupCUDA + RenderImage (:153-189, :471-501) as an object.

There is no fallback path: the shared library must exist (``make`` or ``__graft_entry__.build()``) or
this module raises at import, and every device call raises :class:`CudabrotError` on a HIP error.
"""

import ctypes as C
import os

import numpy as np

CB_DEFAULT_THREADS = 512 * 512  # cudabrot.cu:20,23
CB_SAMPLES_PER_THREAD = 50  # cudabrot.cu:34
CB_DEFAULT_RNG_SEED = 1337  # cudabrot.cu:37
CB_KERNEL_DEFAULT = 0
CB_KERNEL_SIMPLE = 1
CB_KERNEL_TIMED = 2
CB_KERNEL_FULL_ITERATE = 3
CB_TONE_AUTO, CB_TONE_LUT, CB_TONE_THRESHOLDS = 0, 1, 2
CB_KERNEL_FLAG_BURNING_SHIP = 0x100
CB_KERNEL_FLAG_DRAIN = 0x200
CB_KERNEL_FLAG_ANTI = 0x400  # the anti-Buddhabrot (with CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE; no channels)
CB_POWER_MIN, CB_POWER_MAX = 3, 8  # the Multibrot step z^d + c (projected renders only)
CB_KERNEL_POWER_MASK = 0xF000


def CB_KERNEL_POWER(degree):
    """The kernel-variant field of the Multibrot degree (OR-ed into CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE)."""
    degree = int(degree)
    if not CB_POWER_MIN <= degree <= CB_POWER_MAX:
        raise ValueError("degree must be an integer from %d to %d" % (CB_POWER_MIN, CB_POWER_MAX))
    return degree << 12


# the formula steps (include/cudabrot_amd.h, "Formula step"; projected, Julia and palette renders only)
CB_FORMULA_TRICORN, CB_FORMULA_CELTIC, CB_FORMULA_BUFFALO, CB_FORMULA_PERPENDICULAR, CB_FORMULA_CELTIC_TRICORN = 1, 2, 3, 4, 5
CB_FORMULA_MAX = 5
CB_KERNEL_FORMULA_MASK = 0xF0000
CB_FORMULA_NAMES = {"tricorn": 1, "celtic": 2, "buffalo": 3, "perpendicular": 4, "celtic-tricorn": 5}  # the CLI's names


def CB_KERNEL_FORMULA(formula):
    """The kernel-variant field of a formula step (OR-ed into CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE): a code
    CB_FORMULA_TRICORN .. CB_FORMULA_MAX, or one of CB_FORMULA_NAMES."""
    code = CB_FORMULA_NAMES.get(formula) if isinstance(formula, str) else int(formula)
    if code is None or not CB_FORMULA_TRICORN <= code <= CB_FORMULA_MAX:
        raise ValueError("formula must be a code from %d to %d or one of %s" % (CB_FORMULA_TRICORN, CB_FORMULA_MAX,
                                                                                 ", ".join(CB_FORMULA_NAMES)))
    return code << 16


CB_FOCUS_MIN_LEVEL, CB_FOCUS_MAX_LEVEL = 4, 10  # focused render: cells of side 2^-level
CB_ERROR_KERNEL_INVARIANT, CB_ERROR_FOCUS_EMPTY = 100001, 100002
CB_ERROR_AIM_EMPTY = 100003  # cb_renderer_set_aim: the probe marked no cell
# cb_counters.status bits (include/cudabrot_amd.h)
CB_STATUS_QUEUE_OVERFLOW, CB_STATUS_REPLAY_RUNAWAY, CB_STATUS_INTERIOR_MAP, CB_STATUS_CARRY_FOREIGN = 1, 2, 4, 8
CB_COMPOSE_RGB, CB_COMPOSE_HSL = 0, 1
CB_PALETTE_MAX_ENTRIES, CB_PALETTE_MAX_STOPS = 1 << 24, 16  # palette render: the table's entries, the stops of one
CB_DEPTH_MAX_SLICES = 256  # depth render: the planes of one
CB_DENSITY_MAX_RADIUS = 8  # density filter: the widest kernel
CB_PERIOD_MAX_ENTRIES = 1024  # period-palette render: the table's entries (periods 0 .. 1023)
CB_FRAMES_MAX = 256  # frames render: the matrices (and planes) of one
CB_LOCAL_EQUALIZE_MAX_TILES = 16  # locally equalised image: the tiles of one side
LOCAL_EQUALIZE_CLIP_Q = 4 * 256  # ... and the clip the binary takes by default, in 1/256ths

_HERE = os.path.dirname(os.path.abspath(__file__))


def library_path():
    return os.path.join(_HERE, "libcudabrot_amd.so")


class CudabrotError(RuntimeError):
    """A C-ABI call returned a nonzero hipError_t."""

    def __init__(self, code, what):
        self.code = int(code)
        super().__init__("%s failed: HIP error %d (%s)" % (what, self.code, _error_string(self.code)))


class FractalDimensions(C.Structure):
    """cb_fractal_dimensions == FractalDimensions (cudabrot.cu:46-58)."""

    _fields_ = [
        ("w", C.c_int),
        ("h", C.c_int),
        ("min_real", C.c_double),
        ("min_imag", C.c_double),
        ("max_real", C.c_double),
        ("max_imag", C.c_double),
        ("delta_real", C.c_double),
        ("delta_imag", C.c_double),
    ]

    @classmethod
    def make(cls, w, h, min_real=-2.0, max_real=2.0, min_imag=-2.0, max_imag=2.0):
        d = cls(w, h, min_real, min_imag, max_real, max_imag, 0.0, 0.0)
        ok, msg = recompute_pixel_deltas(d)
        if not ok:
            raise ValueError(msg)
        return d


class IterationControl(C.Structure):
    """cb_iteration_control == IterationControl (cudabrot.cu:62-67)."""

    _fields_ = [("max_escape_iterations", C.c_int), ("min_escape_iterations", C.c_int)]


class ColorParams(C.Structure):
    """cb_color_params: the composition and the levels' percentages of the colour stage."""

    _fields_ = [("compose", C.c_int), ("black_percent", C.c_double), ("white_percent", C.c_double),
                ("hue_shift", C.c_double)]

    @classmethod
    def make(cls, compose="rgb", stretch=(2.0, 1.0), hue_shift=0.0):
        if isinstance(compose, str):
            modes = {"rgb": CB_COMPOSE_RGB, "hsl": CB_COMPOSE_HSL}
            if compose not in modes:
                raise ValueError("compose must be 'rgb' or 'hsl', not %r" % compose)
            compose = modes[compose]
        black, white = stretch
        return cls(int(compose), float(black), float(white), float(hue_shift))


class PaletteStop(C.Structure):
    """cb_palette_stop: one colour stop (k, r, g, b) of a palette."""

    _fields_ = [("k", C.c_int), ("r", C.c_int), ("g", C.c_int), ("b", C.c_int)]


DEPTH_AXES = {"zr": 0, "zi": 1, "cr": 2, "ci": 3}  # the CLI's names of the columns of a row


class Depth(C.Structure):
    """cb_depth: the depth row, the window [min, max) and the number of slices of a depth render."""

    _fields_ = [("row", C.c_double * 4), ("min", C.c_double), ("max", C.c_double), ("slices", C.c_int)]

    @classmethod
    def make(cls, row, lo, hi, slices=1):
        """row: an axis name (zr, zi, cr, ci) or four numbers over (z_re, z_im, c_re, c_im)."""
        if isinstance(row, str):
            if row not in DEPTH_AXES:
                raise ValueError("a depth axis is one of %s" % ", ".join(DEPTH_AXES))
            row = [1.0 if j == DEPTH_AXES[row] else 0.0 for j in range(4)]
        v = np.asarray(row, dtype=np.float64).reshape(-1)
        if v.size != 4:
            raise ValueError("a depth row is four numbers: D[4]")
        return cls((C.c_double * 4)(*[float(x) for x in v]), float(lo), float(hi), int(slices))

    def as_tuple(self):
        return tuple(float(x) for x in self.row), float(self.min), float(self.max), int(self.slices)


def _depth(depth):
    """A Depth from a Depth or from (row, min, max[, slices])."""
    return depth if isinstance(depth, Depth) else Depth.make(*depth)


class Counters(C.Structure):
    """cb_counters: exact device-side workload counters."""

    _fields_ = [
        (n, C.c_uint64)
        for n in (
            "samples",
            "rejected",
            "never_escaped",
            "too_fast",
            "recorded",
            "iterate_steps",
            "replay_steps",
            "increments",
            "skipped_steps",
            "status",
            "cycles_head",
            "cycles_long",
            "cycles_replay",
            "cycles_total",
            "rt_not_first_start",
            "rt_last_end",
            "rt_wave_life_sum",
        )
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ScatterArray(C.Structure):
    """cb_scatter_array: one array of the scatter workspace, as bytes from its start."""

    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64)]


SCATTER_ARRAYS = ("wave_count stream a_count a_base grouped region_start region_count region_group owner_first "
                  "group_first group_regions n_regions chunk_desc chunk_list run_start slice_base sorted").split()


class ScatterLayout(C.Structure):
    """cb_scatter_layout: the carve of a scatter workspace (cb_debug_scatter_layout)."""

    _fields_ = [
        (n, C.c_uint32)
        for n in ("enabled n_waves cap n_tiles tiles_x tiles_y n_planes two_level n_groups chunked chunks_per_wave "
                  "max_regions e_row_shift e_col_mask e_row_mask e_chan_shift e_chan_mask reserved").split()
    ] + [(n, ScatterArray) for n in SCATTER_ARRAYS]

    def arrays(self):
        """{name: (offset, bytes)} of the arrays the layout has."""
        return {n: (int(getattr(self, n).offset), int(getattr(self, n).bytes))
                for n in SCATTER_ARRAYS if getattr(self, n).bytes}


def _share_torch_hip_runtime():
    """One HIP runtime per process.

    The PyTorch wheel bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and links it by the
    unversioned file name, so a process that loads /opt/rocm's copy through this library and then
    uses torch.cuda ends up with two HIP/HSA runtimes, and the second one finds no GPU.  Loading
    torch's copy first (globally) makes this library's DT_NEEDED ``libamdhip64.so.7`` resolve to it,
    and a later ``import torch`` finds the same file.  Without torch installed (or with
    CUDABROT_AMD_SYSTEM_HIP=1) the system runtime is used, as the `cudabrot` binary always does.
    """
    if os.environ.get("CUDABROT_AMD_SYSTEM_HIP") == "1":
        return None
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return cand


def _load():
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            "cudabrot_amd: %s is missing -- build it with `make` (or __graft_entry__.build()); "
            "there is no CPU fallback" % path
        )
    _share_torch_hip_runtime()
    lib_ = C.CDLL(path)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    dims_p, it_p, cnt_p = C.POINTER(FractalDimensions), C.POINTER(IterationControl), C.POINTER(Counters)
    col_p = C.POINTER(ColorParams)
    depth_p = C.POINTER(Depth)
    sigs = {
        "cb_abi_version": (i32, []),
        "cb_error_string": (C.c_char_p, [i32]),
        "cb_debug_knob": (C.c_char_p, [C.c_char_p]),
        "cb_debug_last_draw_kernel": (i32, []),
        "cb_debug_interior_map_level": (i32, []),
        "cb_renderer_interior_map_level": (i32, [vp]),
        "cb_recompute_pixel_deltas": (i32, [dims_p, C.POINTER(C.c_char_p)]),
        "cb_rng_state_bytes": (C.c_size_t, [u32]),
        "cb_initialize_rng": (i32, [u64, u64, u32, vp, vp]),
        "cb_scatter_workspace_bytes": (C.c_size_t, [dims_p, u32, u32]),
        "cb_scatter_workspace_bytes_channels": (C.c_size_t, [dims_p, i32, u32, u32]),
        "cb_draw_buddhabrot": (i32, [dims_p, vp, it_p, vp, u32, u32, vp, i32, vp, C.c_size_t, vp, vp]),
        "cb_carry_bytes": (C.c_size_t, [u32]),
        "cb_draw_buddhabrot_channels": (i32, [dims_p, vp, it_p, i32, vp, u32, u32, vp, i32, vp, C.c_size_t, vp, vp]),
        "cb_flush_scatter_channels": (i32, [dims_p, vp, i32, u32, vp, C.c_size_t, vp]),
        "cb_renderer_finish": (i32, [vp]),
        "cb_flush_scatter": (i32, [dims_p, vp, u32, vp, C.c_size_t, vp]),
        "cb_debug_scatter_layout": (i32, [dims_p, i32, u32, vp, C.c_size_t, C.POINTER(ScatterLayout)]),
        "cb_renderer_create": (i32, [C.POINTER(vp), i32, dims_p, it_p, u64, u64, u32]),
        "cb_renderer_create_channels": (i32, [C.POINTER(vp), i32, dims_p, it_p, i32, u64, u64, u32]),
        "cb_renderer_grayscale_plane": (i32, [vp, i32, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_renderer_render_passes": (i32, [vp, u32, i32]),
        "cb_renderer_prepare": (i32, [vp, i32]),
        "cb_renderer_read_histogram": (i32, [vp, vp]),
        "cb_renderer_write_histogram": (i32, [vp, vp]),
        "cb_renderer_read_counters": (i32, [vp, cnt_p]),
        "cb_renderer_read_rng_states": (i32, [vp, vp]),
        "cb_renderer_write_rng_states": (i32, [vp, vp]),
        "cb_renderer_device_histogram": (vp, [vp]),
        "cb_renderers_reduce": (i32, [C.POINTER(vp), i32]),
        "cb_renderer_destroy": (None, [vp]),
        "cb_set_grayscale_pixels": (None, [vp, i32, i32, C.c_double, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_save_image": (i32, [C.c_char_p, vp, i32, i32]),
        "cb_save_image_be": (i32, [C.c_char_p, vp, i32, i32]),
        "cb_tone_value": (C.c_uint16, [u64, u64, C.c_double]),
        "cb_tone_map_device": (i32, [vp, i32, i32, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double), vp]),
        "cb_renderer_grayscale_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_compose_color": (i32, [C.POINTER(vp), i32, i32, col_p, vp, vp]),
        "cb_compose_color_device": (i32, [C.POINTER(vp), i32, i32, C.c_double, i32, col_p, vp, vp, vp]),
        "cb_renderer_color_image": (i32, [vp, C.POINTER(i32), C.c_double, i32, col_p, vp, vp]),
        "cb_save_ppm_be": (i32, [C.c_char_p, vp, i32, i32]),
        "cb_focus_mask_bytes": (C.c_size_t, [i32]),
        "cb_focus_probe": (i32, [dims_p, it_p, vp, u32, u32, i32, vp, vp, i32, vp]),
        "cb_focus_cells": (i32, [i32, vp, i32, vp, C.POINTER(u32)]),
        "cb_draw_buddhabrot_focus": (i32, [dims_p, vp, it_p, vp, u32, u32, vp, i32, i32, vp, u32, vp]),
        "cb_renderer_set_focus": (i32, [vp, i32, u32, i32, i32]),
        "cb_renderer_focus_cells": (i32, [vp, C.POINTER(u32), C.POINTER(u32)]),
        "cb_draw_buddhabrot_projected": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), vp, u32, u32, vp, i32, vp]),
        "cb_renderer_set_projection": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_renderer_projection": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_draw_buddhabrot_julia": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, u32, u32,
                                           vp, i32, vp]),
        "cb_renderer_set_julia": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "cb_renderer_julia": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_palette_from_stops": (i32, [C.POINTER(PaletteStop), i32, vp, u32]),
        "cb_draw_buddhabrot_palette": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, u32, vp,
                                             u32, u32, vp, i32, vp]),
        "cb_renderer_set_palette": (i32, [vp, vp, u32]),
        "cb_renderer_palette": (i32, [vp, C.POINTER(u32)]),
        "cb_renderer_palette_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_draw_buddhabrot_phoenix": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), vp, u32, u32, vp, i32, vp]),
        "cb_renderer_set_phoenix": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_renderer_phoenix": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_draw_buddhabrot_bounded": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, u32, u32,
                                             vp, i32, vp]),
        "cb_aim_probe": (i32, [dims_p, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, vp, u32, u32, i32, vp, vp,
                               i32, vp]),
        "cb_draw_buddhabrot_aimed": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, vp, u32, u32,
                                           vp, i32, i32, vp, u32, vp]),
        "cb_renderer_set_aim": (i32, [vp, i32, u32, i32, i32]),
        "cb_renderer_aim_cells": (i32, [vp, C.POINTER(u32), C.POINTER(u32)]),
        "cb_renderer_set_bounded": (i32, [vp]),
        "cb_renderer_bounded": (i32, [vp]),
        "cb_draw_buddhabrot_periods": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, u32,
                                             C.c_double, vp, u32, u32, vp, i32, vp]),
        "cb_renderer_set_period_palette": (i32, [vp, vp, u32, C.c_double]),
        "cb_renderer_period_palette": (i32, [vp, C.POINTER(u32), C.POINTER(C.c_double)]),
        "cb_renderer_period_palette_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_draw_buddhabrot_depth": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), depth_p, vp, u32,
                                           u32, vp, i32, vp]),
        "cb_renderer_set_depth": (i32, [vp, depth_p]),
        "cb_renderer_depth": (i32, [vp, depth_p]),
        "cb_renderer_depth_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_draw_buddhabrot_depth_palette": (i32, [dims_p, vp, it_p, C.POINTER(C.c_double), C.POINTER(C.c_double), depth_p,
                                                   vp, u32, vp, u32, u32, vp, i32, vp]),
        "cb_renderer_set_depth_palette": (i32, [vp, depth_p, vp, u32]),
        "cb_renderer_depth_palette": (i32, [vp, depth_p, C.POINTER(u32)]),
        "cb_renderer_depth_palette_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_rotate_projection": (i32, [C.POINTER(C.c_double), i32, i32, C.c_double]),
        "cb_frames_from_sweep": (i32, [C.POINTER(C.c_double), i32, i32, C.c_double, C.c_double, i32, vp, vp]),
        "cb_draw_buddhabrot_frames": (i32, [dims_p, vp, it_p, vp, i32, C.POINTER(C.c_double), vp, u32, u32, vp, i32, vp]),
        "cb_renderer_set_frames": (i32, [vp, vp, i32]),
        "cb_renderer_frames": (i32, [vp, vp]),
        "cb_renderer_frames_image": (i32, [vp, C.c_double, i32, vp, C.POINTER(u64), C.POINTER(C.c_double)]),
        "cb_white_clip_ok": (i32, [C.c_double]),
        "cb_white_rank": (u64, [u64, C.c_double]),
        "cb_white_count": (i32, [vp, u64, C.c_double, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "cb_set_grayscale_pixels_white": (i32, [vp, i32, i32, C.c_double, C.c_double, vp, C.POINTER(u64),
                                                C.POINTER(C.c_double), C.POINTER(u64)]),
        "cb_white_count_device": (i32, [vp, u64, C.c_double, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]),
        "cb_tone_map_device_white": (i32, [vp, i32, i32, C.c_double, i32, C.c_double, vp, C.POINTER(u64),
                                           C.POINTER(C.c_double), C.POINTER(u64), vp]),
        "cb_renderer_set_white_clip": (i32, [vp, C.c_double]),
        "cb_renderer_white_clip": (i32, [vp, C.POINTER(C.c_double)]),
        "cb_renderer_last_white": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "cb_density_thresholds": (i32, [i32, C.c_double, u64, C.POINTER(u64)]),
        "cb_density_arguments_ok": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(u64), vp]),
        "cb_density_filter": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(u64), vp]),
        "cb_density_filter_device": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(u64), vp, vp]),
        "cb_renderer_set_density_filter": (i32, [vp, i32, C.c_double, u64]),
        "cb_renderer_density_filter": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(u64)]),
        "cb_equalize_key": (u32, [u64]),
        "cb_equalize_bins": (i32, [vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]),
        "cb_equalize_table": (i32, [vp, C.c_double, vp, C.POINTER(u64), C.POINTER(u64)]),
        "cb_set_grayscale_pixels_equalized": (i32, [vp, i32, i32, C.c_double, vp, C.POINTER(u64), C.POINTER(C.c_double),
                                                    C.POINTER(u64)]),
        "cb_equalize_bins_device": (i32, [vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]),
        "cb_tone_map_device_equalized": (i32, [vp, i32, i32, C.c_double, vp, C.POINTER(u64), C.POINTER(C.c_double),
                                               C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]),
        "cb_renderer_set_equalize": (i32, [vp, i32]),
        "cb_renderer_equalize": (i32, [vp]),
        "cb_renderer_last_equalize": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "cb_local_equalize_ok": (i32, [i32, i32, i32, i32, i32, u32]),
        "cb_local_equalize_bins": (i32, [vp, i32, i32, i32, i32, i32, vp, C.POINTER(u64), C.POINTER(u64)]),
        "cb_local_equalize_clip": (i32, [vp, u32, vp, C.POINTER(u64)]),
        "cb_set_grayscale_pixels_local_equalized": (i32, [vp, i32, i32, i32, i32, i32, u32, C.c_double, vp, C.POINTER(u64),
                                                          C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64),
                                                          C.POINTER(u64)]),
        "cb_local_equalize_bins_device": (i32, [vp, i32, i32, i32, i32, i32, vp, C.POINTER(u64), C.POINTER(u64), vp]),
        "cb_tone_map_device_local_equalized": (i32, [vp, i32, i32, i32, i32, i32, u32, C.c_double, vp, C.POINTER(u64),
                                                     C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64),
                                                     vp]),
        "cb_renderer_set_local_equalize": (i32, [vp, i32, i32, u32]),
        "cb_renderer_local_equalize": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32)]),
        "cb_renderer_last_local_equalize": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib_, name)  # AttributeError here = the library does not export the ABI
        fn.restype = res
        fn.argtypes = args
    return lib_


lib = _load()
EXPORTED_SYMBOLS = (
    "cb_abi_version cb_error_string cb_debug_knob cb_debug_last_draw_kernel cb_debug_interior_map_level cb_renderer_interior_map_level cb_recompute_pixel_deltas cb_rng_state_bytes cb_initialize_rng "
    "cb_scatter_workspace_bytes cb_scatter_workspace_bytes_channels cb_carry_bytes cb_draw_buddhabrot cb_flush_scatter cb_renderer_create "
    "cb_renderer_render_passes cb_renderer_finish "
    "cb_renderer_read_histogram "
    "cb_renderer_write_histogram cb_renderer_read_counters cb_renderer_device_histogram "
    "cb_renderer_destroy cb_set_grayscale_pixels cb_save_image cb_save_image_be cb_tone_value "
    "cb_tone_map_device cb_renderer_grayscale_image cb_renderer_read_rng_states cb_renderer_write_rng_states "
    "cb_draw_buddhabrot_channels cb_flush_scatter_channels cb_renderer_create_channels cb_renderer_grayscale_plane cb_renderers_reduce "
    "cb_renderer_prepare cb_compose_color cb_compose_color_device cb_renderer_color_image cb_save_ppm_be "
    "cb_focus_mask_bytes cb_focus_probe cb_focus_cells cb_draw_buddhabrot_focus cb_renderer_set_focus cb_renderer_focus_cells "
    "cb_draw_buddhabrot_projected cb_renderer_set_projection cb_renderer_projection cb_debug_scatter_layout "
    "cb_draw_buddhabrot_julia cb_renderer_set_julia cb_renderer_julia "
    "cb_palette_from_stops cb_draw_buddhabrot_palette cb_renderer_set_palette cb_renderer_palette cb_renderer_palette_image "
    "cb_draw_buddhabrot_depth cb_renderer_set_depth cb_renderer_depth cb_renderer_depth_image "
    "cb_draw_buddhabrot_depth_palette cb_renderer_set_depth_palette cb_renderer_depth_palette "
    "cb_renderer_depth_palette_image "
    "cb_draw_buddhabrot_phoenix cb_renderer_set_phoenix cb_renderer_phoenix "
    "cb_draw_buddhabrot_bounded cb_renderer_set_bounded cb_renderer_bounded "
    "cb_aim_probe cb_draw_buddhabrot_aimed cb_renderer_set_aim cb_renderer_aim_cells "
    "cb_draw_buddhabrot_periods cb_renderer_set_period_palette cb_renderer_period_palette "
    "cb_renderer_period_palette_image "
    "cb_rotate_projection cb_frames_from_sweep cb_draw_buddhabrot_frames cb_renderer_set_frames cb_renderer_frames "
    "cb_renderer_frames_image "
    "cb_white_clip_ok cb_white_rank cb_white_count cb_set_grayscale_pixels_white cb_white_count_device "
    "cb_tone_map_device_white cb_renderer_set_white_clip cb_renderer_white_clip cb_renderer_last_white "
    "cb_density_thresholds cb_density_arguments_ok cb_density_filter cb_density_filter_device "
    "cb_renderer_set_density_filter cb_renderer_density_filter "
    "cb_equalize_key cb_equalize_bins cb_equalize_table cb_set_grayscale_pixels_equalized cb_equalize_bins_device "
    "cb_tone_map_device_equalized cb_renderer_set_equalize cb_renderer_equalize cb_renderer_last_equalize "
    "cb_local_equalize_ok cb_local_equalize_bins cb_local_equalize_clip cb_set_grayscale_pixels_local_equalized "
    "cb_local_equalize_bins_device cb_tone_map_device_local_equalized cb_renderer_set_local_equalize "
    "cb_renderer_local_equalize cb_renderer_last_local_equalize"
).split()


def _error_string(code):
    return lib.cb_error_string(int(code)).decode()


def _check(code, what):
    if code != 0:
        raise CudabrotError(code, what)


def recompute_pixel_deltas(dims):
    """RecomputePixelDeltas (cudabrot.cu:505-527) -> (ok, message-or-None); fills dims.delta_*."""
    msg = C.c_char_p()
    ok = lib.cb_recompute_pixel_deltas(C.byref(dims), C.byref(msg))
    return bool(ok), (None if ok else msg.value.decode())


def rng_state_bytes(n_threads):
    return int(lib.cb_rng_state_bytes(n_threads))


def initialize_rng(seed, first_subsequence, n_threads, d_states, stream=0):
    """InitializeRNG (cudabrot.cu:146-149,179) on caller-owned device memory (integer pointers)."""
    _check(lib.cb_initialize_rng(seed, first_subsequence, n_threads, d_states, stream), "cb_initialize_rng")


def scatter_workspace_bytes(dims, n_threads, samples_per_thread, n_channels=1):
    """Suggested scatter-workspace size for launches of this shape (0: the canvas cannot use one);
    n_channels > 1: for a fused multi-channel launch of that many planes."""
    return int(lib.cb_scatter_workspace_bytes_channels(C.byref(dims), n_channels, n_threads, samples_per_thread))


def carry_bytes(n_threads):
    """Size of the carry buffer (in-flight orbits handed from launch to launch)."""
    return int(lib.cb_carry_bytes(n_threads))


def draw_buddhabrot(dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters=0,
                    kernel_variant=CB_KERNEL_DEFAULT, stream=0, d_workspace=0, workspace_bytes=0, d_carry=0):
    """DrawBuddhabrot (cudabrot.cu:379-414,485-486) on caller-owned device memory; asynchronous.
    With a workspace the increments go through the deferred tile-binned scatter, else direct atomics.
    With a (zeroed) carry buffer, orbits still in flight are handed to the next call; a last call with
    samples_per_thread=0 completes them."""
    _check(
        lib.cb_draw_buddhabrot(C.byref(dims), d_hist, C.byref(iterations), d_states, n_threads,
                               samples_per_thread, d_counters, kernel_variant, d_workspace, workspace_bytes,
                               d_carry, stream),
        "cb_draw_buddhabrot",
    )


def flush_scatter(dims, d_hist, n_threads, d_workspace, workspace_bytes, stream=0):
    """Adds the pixel stream a draw_buddhabrot call deferred into the workspace to the histogram."""
    _check(lib.cb_flush_scatter(C.byref(dims), d_hist, n_threads, d_workspace, workspace_bytes, stream),
           "cb_flush_scatter")


def debug_scatter_layout(dims, n_threads, d_workspace, workspace_bytes, n_channels=0):
    """Where flush_scatter (n_channels = 0) or flush_scatter_channels (1..4) finds its arrays in this workspace: a
    ScatterLayout.  Host arithmetic on the arguments; d_workspace is any non-zero address and is not touched."""
    out = ScatterLayout()
    _check(lib.cb_debug_scatter_layout(C.byref(dims), n_channels, n_threads, d_workspace, workspace_bytes,
                                       C.byref(out)), "cb_debug_scatter_layout")
    return out


def focus_mask_bytes(level):
    """Bytes of a focus mask of this level: (4 * 2^level)^2 bits (0 for a level out of range)."""
    return int(lib.cb_focus_mask_bytes(int(level)))


def focus_probe(dims, iterations, d_states, n_threads, samples_per_thread, level, d_mask, d_counters=0,
                kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The probe of a focused render on caller-owned device memory (integer pointers); ORs into d_mask."""
    _check(
        lib.cb_focus_probe(C.byref(dims), C.byref(iterations), d_states, n_threads, samples_per_thread, int(level),
                           d_mask, d_counters, kernel_variant, stream),
        "cb_focus_probe",
    )


def focus_cells(level, mask, dilate=1):
    """The cell list of a host mask (u32 words): the mask dilated by `dilate` cells, ascending indices (u32 array)."""
    m = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
    if m.size * 4 != focus_mask_bytes(level):
        raise ValueError("mask size does not match the level")
    n = C.c_uint32()
    _check(lib.cb_focus_cells(int(level), m.ctypes.data, int(dilate), None, C.byref(n)), "cb_focus_cells")
    cells = np.empty(int(n.value), dtype=np.uint32)
    _check(lib.cb_focus_cells(int(level), m.ctypes.data, int(dilate), cells.ctypes.data, C.byref(n)), "cb_focus_cells")
    return cells


def draw_buddhabrot_focus(dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters=0,
                          kernel_variant=CB_KERNEL_DEFAULT, level=0, d_cells=0, n_cells=0, stream=0):
    """The focused draw on caller-owned device memory: samples from d_cells[0 .. n_cells) of the level's grid (level 0,
    no cells: the uniform source, a normal render through the focus kernel)."""
    _check(
        lib.cb_draw_buddhabrot_focus(C.byref(dims), d_hist, C.byref(iterations), d_states, n_threads,
                                     samples_per_thread, d_counters, kernel_variant, int(level), d_cells, n_cells, stream),
        "cb_draw_buddhabrot_focus",
    )


IDENTITY_PROJECTION = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _projection(projection):
    """P[2][4] (rows u, v; columns z_re, z_im, c_re, c_im) as eight C doubles."""
    p = np.asarray(projection, dtype=np.float64).reshape(-1)
    if p.size != 8:
        raise ValueError("a projection is eight numbers: P[2][4]")
    return (C.c_double * 8)(*[float(x) for x in p])


def draw_buddhabrot_projected(dims, d_hist, iterations, projection, d_states, n_threads, samples_per_thread,
                              d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The projected draw on caller-owned device memory (cb_draw_buddhabrot_projected): the normal sample stream, every
    recorded point plotted at P (z_re, z_im, c_re, c_im); the canvas is the (u, v) window."""
    _check(
        lib.cb_draw_buddhabrot_projected(C.byref(dims), d_hist, C.byref(iterations), _projection(projection), d_states,
                                         n_threads, samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_projected",
    )


def _julia_c(c):
    """The fixed c of a Julia render, (c_re, c_im), as two C doubles."""
    v = np.asarray(c, dtype=np.float64).reshape(-1)
    if v.size != 2:
        raise ValueError("a Julia parameter is two numbers: (c_re, c_im)")
    return (C.c_double * 2)(float(v[0]), float(v[1]))


def draw_buddhabrot_julia(dims, d_hist, iterations, projection, julia_c, d_states, n_threads, samples_per_thread,
                          d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The Julia draw on caller-owned device memory (cb_draw_buddhabrot_julia): the sample of the normal stream is z_0,
    c = julia_c is fixed, every recorded point is plotted at P (z_re, z_im, c_re, c_im)."""
    _check(
        lib.cb_draw_buddhabrot_julia(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                     _julia_c(julia_c), d_states, n_threads, samples_per_thread, d_counters,
                                     kernel_variant, stream),
        "cb_draw_buddhabrot_julia",
    )


def _phoenix_p(p):
    """The parameter of a Phoenix render, (p_re, p_im), as two C doubles."""
    v = np.asarray(p, dtype=np.float64).reshape(-1)
    if v.size != 2:
        raise ValueError("a Phoenix parameter is two numbers: (p_re, p_im)")
    return (C.c_double * 2)(float(v[0]), float(v[1]))


def draw_buddhabrot_phoenix(dims, d_hist, iterations, projection, julia_c, phoenix_p, d_states, n_threads,
                            samples_per_thread, d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The Phoenix draw on caller-owned device memory (cb_draw_buddhabrot_phoenix): the step z^2 + c + p z_prev;
    julia_c None samples c (z_0 = c), else c is fixed and the sample is z_0.  One plane."""
    _check(
        lib.cb_draw_buddhabrot_phoenix(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                       None if julia_c is None else _julia_c(julia_c), _phoenix_p(phoenix_p), d_states,
                                       n_threads, samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_phoenix",
    )


def draw_buddhabrot_bounded(dims, d_hist, iterations, projection, julia_c, d_states, n_threads, samples_per_thread,
                            d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The bounded draw on caller-owned device memory (cb_draw_buddhabrot_bounded): the orbits that never escape, z_1 ..
    z_max, plotted at P (z_re, z_im, c_re, c_im); julia_c None samples c (z_0 = c), else c is fixed and the sample is z_0.
    One plane."""
    _check(
        lib.cb_draw_buddhabrot_bounded(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                       None if julia_c is None else _julia_c(julia_c), d_states, n_threads,
                                       samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_bounded",
    )


def aim_probe(dims, iterations, projection, julia_c, bounded, d_states, n_threads, samples_per_thread, level, d_mask,
              d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The probe of an aimed render on caller-owned device memory (cb_aim_probe): the un-aimed render -- projected or, with
    bounded, bounded; julia_c None samples c -- on the normal stream, which ORs into d_mask the cells of the sample plane
    whose samples have a plotted orbit point on the canvas."""
    _check(
        lib.cb_aim_probe(C.byref(dims), C.byref(iterations), _projection(projection),
                         None if julia_c is None else _julia_c(julia_c), 1 if bounded else 0, d_states, n_threads,
                         samples_per_thread, int(level), d_mask, d_counters, kernel_variant, stream),
        "cb_aim_probe",
    )


def draw_buddhabrot_aimed(dims, d_hist, iterations, projection, julia_c, bounded, d_states, n_threads, samples_per_thread,
                          d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, level=0, d_cells=0, n_cells=0, stream=0):
    """The aimed draw on caller-owned device memory (cb_draw_buddhabrot_aimed): the projected or bounded render with its
    samples from d_cells[0 .. n_cells) of the level's grid (level 0, no cells: the uniform source, the un-aimed render
    through the aim kernel)."""
    _check(
        lib.cb_draw_buddhabrot_aimed(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                     None if julia_c is None else _julia_c(julia_c), 1 if bounded else 0, d_states,
                                     n_threads, samples_per_thread, d_counters, kernel_variant, int(level), d_cells, n_cells,
                                     stream),
        "cb_draw_buddhabrot_aimed",
    )


def draw_buddhabrot_periods(dims, d_hist, iterations, projection, julia_c, d_lut, n_entries, period_eps, d_states,
                            n_threads, samples_per_thread, d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The period-palette draw on caller-owned device memory (cb_draw_buddhabrot_periods): the bounded draw into three
    planes, each bounded orbit in the colour d_lut (n_entries entries, 2 .. CB_PERIOD_MAX_ENTRIES, on the device) has for
    its period: the least j <= n_entries - 1 with |z_{max+j} - z_max|^2 <= period_eps, 0 if there is none."""
    _check(
        lib.cb_draw_buddhabrot_periods(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                       None if julia_c is None else _julia_c(julia_c), d_lut, n_entries, period_eps,
                                       d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_periods",
    )


def palette_from_stops(stops, n_entries):
    """The table of a list of colour stops (cb_palette_from_stops): stops = [(k, r, g, b), ...], k ascending -> u32 array
    of n_entries entries, entry k = r | g << 8 | b << 16 of an orbit with escape index k."""
    stops = [tuple(int(v) for v in s) for s in stops]
    if any(len(s) != 4 for s in stops):
        raise ValueError("a colour stop is four numbers: (k, r, g, b)")
    arr = (PaletteStop * max(len(stops), 1))(*[PaletteStop(*s) for s in stops])
    lut = np.empty(max(int(n_entries), 0), dtype=np.uint32)
    _check(lib.cb_palette_from_stops(arr, len(stops), lut.ctypes.data, int(n_entries) & 0xFFFFFFFF), "cb_palette_from_stops")
    return lut


def draw_buddhabrot_palette(dims, d_hist, iterations, projection, julia_c, d_lut, n_entries, d_states, n_threads,
                            samples_per_thread, d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The palette draw on caller-owned device memory (cb_draw_buddhabrot_palette): d_hist is three planes, d_lut the table
    of n_entries == max_iter entries on the device; julia_c None samples c (a projected render), else c is fixed."""
    _check(
        lib.cb_draw_buddhabrot_palette(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                       None if julia_c is None else _julia_c(julia_c), d_lut, n_entries, d_states,
                                       n_threads, samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_palette",
    )


def draw_buddhabrot_depth(dims, d_hist, iterations, projection, julia_c, depth, d_states, n_threads, samples_per_thread,
                          d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The depth draw on caller-owned device memory (cb_draw_buddhabrot_depth): d_hist is depth.slices planes; depth is a
    Depth or (row, min, max[, slices]); julia_c None samples c (a projected render), else c is fixed."""
    _check(
        lib.cb_draw_buddhabrot_depth(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                     None if julia_c is None else _julia_c(julia_c), C.byref(_depth(depth)), d_states,
                                     n_threads, samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_depth",
    )


def draw_buddhabrot_depth_palette(dims, d_hist, iterations, projection, julia_c, depth, d_lut, n_entries, d_states,
                                  n_threads, samples_per_thread, d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The depth-palette draw on caller-owned device memory (cb_draw_buddhabrot_depth_palette): d_hist is three planes,
    d_lut the table of n_entries == depth.slices entries on the device; depth is a Depth or (row, min, max[, slices]);
    julia_c None samples c (a projected render), else c is fixed."""
    _check(
        lib.cb_draw_buddhabrot_depth_palette(C.byref(dims), d_hist, C.byref(iterations), _projection(projection),
                                             None if julia_c is None else _julia_c(julia_c), C.byref(_depth(depth)), d_lut,
                                             n_entries, d_states, n_threads, samples_per_thread, d_counters, kernel_variant,
                                             stream),
        "cb_draw_buddhabrot_depth_palette",
    )


def _frames(frames):
    """The matrices of a frames render, F x P[2][4], as a contiguous float64 array [F, 8]."""
    a = np.ascontiguousarray(frames, dtype=np.float64)
    if a.size == 0 or a.size % 8 != 0:
        raise ValueError("frames are F matrices of eight numbers each: P[2][4]")
    return a.reshape(-1, 8)


def frames_from_sweep(base, axes, deg0, deg1, n_frames):
    """The matrices of a rotation sweep (cb_frames_from_sweep): base rotated in the coordinate plane axes = (X, Y) -- names
    of DEPTH_AXES or columns 0 .. 3 -- by a_f = deg0 + ((deg1 - deg0) * f) / n_frames -> (matrices [F, 8], angles [F])."""
    x, y = (DEPTH_AXES.get(a, a) if isinstance(a, str) else a for a in axes)
    if isinstance(x, str) or isinstance(y, str):
        raise ValueError("a sweep axis is one of %s" % ", ".join(DEPTH_AXES))
    n = int(n_frames)
    out = np.empty((max(n, 0), 8), dtype=np.float64)
    angles = np.empty(max(n, 0), dtype=np.float64)
    _check(lib.cb_frames_from_sweep(_projection(base), int(x), int(y), float(deg0), float(deg1), n, out.ctypes.data,
                                    angles.ctypes.data), "cb_frames_from_sweep")
    return out, angles


def draw_buddhabrot_frames(dims, d_hist, iterations, d_frames, n_frames, julia_c, d_states, n_threads, samples_per_thread,
                           d_counters=0, kernel_variant=CB_KERNEL_DEFAULT, stream=0):
    """The frames draw on caller-owned device memory (cb_draw_buddhabrot_frames): d_hist is n_frames planes, d_frames the
    n_frames matrices (8 doubles each) on the device; julia_c None samples c (a projected render), else c is fixed."""
    _check(
        lib.cb_draw_buddhabrot_frames(C.byref(dims), d_hist, C.byref(iterations), d_frames, int(n_frames),
                                      None if julia_c is None else _julia_c(julia_c), d_states, n_threads,
                                      samples_per_thread, d_counters, kernel_variant, stream),
        "cb_draw_buddhabrot_frames",
    )


class Renderer:
    """SetupCUDA + RenderImage (cudabrot.cu:153-189, 471-501) over the C ABI's cb_renderer."""

    def __init__(self, dims, iterations, device=0, seed=CB_DEFAULT_RNG_SEED, first_subsequence=0,
                 n_threads=CB_DEFAULT_THREADS):
        """iterations: an IterationControl, or -- fused multi-channel render (N2) -- a list of (max, min)
        windows; read_histogram then returns one plane per window ([k, h, w])."""
        self.dims = dims
        self.iterations = iterations
        self.n_threads = n_threads
        self._h = C.c_void_p()
        if isinstance(iterations, IterationControl):
            self.n_channels = 0
            _check(
                lib.cb_renderer_create(C.byref(self._h), device, C.byref(dims), C.byref(iterations), seed,
                                       first_subsequence, n_threads),
                "cb_renderer_create",
            )
        else:
            self.n_channels = len(iterations)
            arr = (IterationControl * len(iterations))(*[IterationControl(int(m), int(c)) for m, c in iterations])
            _check(
                lib.cb_renderer_create_channels(C.byref(self._h), device, C.byref(dims), arr, len(iterations), seed,
                                                first_subsequence, n_threads),
                "cb_renderer_create_channels",
            )

    def _set_cells(self, which, level, probe_passes, dilate, kernel_variant):
        """cb_renderer_set_<which>, then cb_renderer_<which>_cells: the focused and the aimed renderer's setter."""
        name = "cb_renderer_set_" + which
        _check(getattr(lib, name)(self._h, int(level), int(probe_passes), int(dilate), kernel_variant), name)
        return self._cells(which)

    def _cells(self, which):
        name = "cb_renderer_%s_cells" % which
        n, total = C.c_uint32(), C.c_uint32()
        _check(getattr(lib, name)(self._h, C.byref(n), C.byref(total)), name)
        return int(n.value), int(total.value)

    def set_focus(self, level=8, probe_passes=64, dilate=1, kernel_variant=CB_KERNEL_DEFAULT):
        """Make this a focused renderer (cb_renderer_set_focus), before the first pass -> (cells listed, cells of the
        grid).  Raises CudabrotError with code CB_ERROR_FOCUS_EMPTY when the probe marks no cell."""
        return self._set_cells("focus", level, probe_passes, dilate, kernel_variant)

    def focus_cells(self):
        """(cells listed, cells of the grid) of a focused renderer; (0, 0) without focus."""
        return self._cells("focus")

    def set_aim(self, level=8, probe_passes=64, dilate=1, kernel_variant=CB_KERNEL_DEFAULT):
        """Make this an aimed renderer (cb_renderer_set_aim), before the first pass -> (cells listed, cells of the grid).
        Raises CudabrotError with code CB_ERROR_AIM_EMPTY when the probe marks no cell."""
        return self._set_cells("aim", level, probe_passes, dilate, kernel_variant)

    def aim_cells(self):
        """(cells listed, cells of the grid) of an aimed renderer; (0, 0) for any other."""
        return self._cells("aim")

    def set_projection(self, projection):
        """Make this a projected renderer (cb_renderer_set_projection), before the first pass."""
        _check(lib.cb_renderer_set_projection(self._h, _projection(projection)), "cb_renderer_set_projection")

    def projection(self):
        """The matrix of a projected renderer as a [2, 4] array; None without one."""
        out = (C.c_double * 8)()
        if not lib.cb_renderer_projection(self._h, out):
            return None
        return np.array(list(out), dtype=np.float64).reshape(2, 4)

    def set_julia(self, julia_c, projection=None):
        """Make this a Julia renderer (cb_renderer_set_julia), before the first pass; projection None: the identity."""
        p = None if projection is None else _projection(projection)
        _check(lib.cb_renderer_set_julia(self._h, p, _julia_c(julia_c)), "cb_renderer_set_julia")

    def julia(self):
        """The c of a Julia renderer as (c_re, c_im); None for any other renderer."""
        out = (C.c_double * 2)()
        if not lib.cb_renderer_julia(self._h, out):
            return None
        return float(out[0]), float(out[1])

    def set_phoenix(self, phoenix_p):
        """Give this renderer the Phoenix step with parameter p (cb_renderer_set_phoenix), before the first pass and after
        set_projection or set_julia.  The histogram stays one plane."""
        _check(lib.cb_renderer_set_phoenix(self._h, _phoenix_p(phoenix_p)), "cb_renderer_set_phoenix")

    def set_bounded(self):
        """Make this a bounded renderer (cb_renderer_set_bounded), before the first pass: the orbits that never escape are
        plotted.  Alone it brings the identity projection; after set_projection or set_julia it keeps theirs.  The
        histogram stays one plane."""
        _check(lib.cb_renderer_set_bounded(self._h), "cb_renderer_set_bounded")

    def bounded(self):
        """Whether this is a bounded renderer."""
        return bool(lib.cb_renderer_bounded(self._h))

    def set_period_palette(self, lut, eps=2.0 ** -66):
        """Make this a period-palette renderer (cb_renderer_set_period_palette), before the first pass, where set_bounded
        is admitted: lut is the table, 2 .. CB_PERIOD_MAX_ENTRIES u32 entries, entry k the colour of the bounded orbits of
        period k (0: no period up to len(lut) - 1); eps the tolerance of the return test.  The histogram becomes three
        planes."""
        a = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
        _check(lib.cb_renderer_set_period_palette(self._h, a.ctypes.data, a.size, float(eps)),
               "cb_renderer_set_period_palette")

    def period_palette(self):
        """(entries of the table, eps) of a period-palette renderer; None for any other renderer."""
        n, eps = C.c_uint32(), C.c_double()
        if not lib.cb_renderer_period_palette(self._h, C.byref(n), C.byref(eps)):
            return None
        return int(n.value), float(eps.value)

    def period_palette_image(self, gamma=1.0, mode=0):
        """The image of a period-palette renderer (cb_renderer_period_palette_image) -> (big-endian u16 image [h,w,3] = the
        PPM body, the largest count of the three planes, scale)."""
        return self._image("cb_renderer_period_palette_image", (self.dims.h, self.dims.w, 3), gamma, mode)

    def phoenix(self):
        """The p of a Phoenix renderer as (p_re, p_im); None for any other renderer."""
        out = (C.c_double * 2)()
        if not lib.cb_renderer_phoenix(self._h, out):
            return None
        return float(out[0]), float(out[1])

    def set_palette(self, lut):
        """Make this a palette renderer (cb_renderer_set_palette), before the first pass and after set_projection or
        set_julia (alone: the identity projection): lut is the table, max_iter u32 entries.  The histogram becomes three
        planes."""
        a = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
        _check(lib.cb_renderer_set_palette(self._h, a.ctypes.data, a.size), "cb_renderer_set_palette")

    def palette(self):
        """The number of entries of a palette renderer's table; None for any other renderer."""
        n = C.c_uint32()
        if not lib.cb_renderer_palette(self._h, C.byref(n)):
            return None
        return int(n.value)

    def palette_image(self, gamma=1.0, mode=0):
        """The image of a palette renderer (cb_renderer_palette_image) -> (big-endian u16 image [h,w,3] = the PPM body,
        the largest count of the three planes, scale)."""
        return self._image("cb_renderer_palette_image", (self.dims.h, self.dims.w, 3), gamma, mode)

    def set_depth(self, depth):
        """Give this renderer a depth (cb_renderer_set_depth), before the first pass and after set_projection or
        set_julia: depth is a Depth or (row, min, max[, slices]).  The histogram becomes `slices` planes."""
        d = _depth(depth)
        _check(lib.cb_renderer_set_depth(self._h, C.byref(d)), "cb_renderer_set_depth")

    def depth(self):
        """The depth of a renderer as a Depth; None for a renderer without one."""
        out = Depth()
        if not lib.cb_renderer_depth(self._h, C.byref(out)):
            return None
        return out

    def depth_image(self, gamma=1.0, mode=0):
        """The image of a renderer with a depth (cb_renderer_depth_image) -> (big-endian u16 images [slices, h, w] = the
        bodies of the PGM sequence, the largest count of all planes, scale)."""
        slices = lib.cb_renderer_depth(self._h, None)
        return self._image("cb_renderer_depth_image", (max(slices, 1), self.dims.h, self.dims.w), gamma, mode)

    def set_depth_palette(self, depth, lut):
        """Give this renderer a depth palette (cb_renderer_set_depth_palette), before the first pass and after
        set_projection or set_julia: depth is a Depth or (row, min, max[, slices]), lut the table, `slices` u32 entries.
        The histogram becomes three planes."""
        d = _depth(depth)
        a = np.ascontiguousarray(lut, dtype=np.uint32).reshape(-1)
        _check(lib.cb_renderer_set_depth_palette(self._h, C.byref(d), a.ctypes.data, a.size), "cb_renderer_set_depth_palette")

    def depth_palette(self):
        """(Depth, entries of the table) of a renderer with a depth palette; None for any other renderer."""
        out, n = Depth(), C.c_uint32()
        if not lib.cb_renderer_depth_palette(self._h, C.byref(out), C.byref(n)):
            return None
        return out, int(n.value)

    def depth_palette_image(self, gamma=1.0, mode=0):
        """The image of a renderer with a depth palette (cb_renderer_depth_palette_image) -> (big-endian u16 image [h,w,3] =
        the PPM body, the largest count of the three planes, scale)."""
        return self._image("cb_renderer_depth_palette_image", (self.dims.h, self.dims.w, 3), gamma, mode)

    def set_frames(self, frames):
        """Give this renderer frames (cb_renderer_set_frames), before the first pass and after set_projection or
        set_julia: frames is F matrices, [F, 8].  The histogram becomes F planes."""
        a = _frames(frames)
        _check(lib.cb_renderer_set_frames(self._h, a.ctypes.data, a.shape[0]), "cb_renderer_set_frames")

    def frames(self):
        """The matrices of a renderer with frames, [F, 8]; None for a renderer without them."""
        n = lib.cb_renderer_frames(self._h, None)
        if not n:
            return None
        out = np.empty((n, 8), dtype=np.float64)
        lib.cb_renderer_frames(self._h, out.ctypes.data)
        return out

    def frames_image(self, gamma=1.0, mode=0):
        """The image of a renderer with frames (cb_renderer_frames_image) -> (big-endian u16 images [F, h, w] = the bodies
        of the PGM sequence, the largest count of all planes, scale)."""
        n = lib.cb_renderer_frames(self._h, None)
        return self._image("cb_renderer_frames_image", (max(n, 1), self.dims.h, self.dims.w), gamma, mode)

    def _image(self, name, shape, gamma, mode):
        """One of the four image calls above into a big-endian u16 buffer of `shape` -> (image, largest count, scale)."""
        out = np.empty(shape, dtype=">u2")
        mx, scale = C.c_uint64(), C.c_double()
        _check(getattr(lib, name)(self._h, float(gamma), int(mode), out.ctypes.data, C.byref(mx), C.byref(scale)), name)
        return out, int(mx.value), float(scale.value)

    def _planes(self):
        """The planes of the histogram, asked of the library; 0: the one plane that read_histogram returns as [h, w]."""
        if (lib.cb_renderer_palette(self._h, None) or lib.cb_renderer_depth_palette(self._h, None, None)
                or lib.cb_renderer_period_palette(self._h, None, None)):
            return 3
        return lib.cb_renderer_depth(self._h, None) or lib.cb_renderer_frames(self._h, None) or self.n_channels

    def prepare(self, kernel_variant=CB_KERNEL_DEFAULT):
        """Allocate now what the first render_passes would (the scatter workspaces)."""
        _check(lib.cb_renderer_prepare(self._h, kernel_variant), "cb_renderer_prepare")

    def render_passes(self, passes, kernel_variant=CB_KERNEL_DEFAULT):
        _check(lib.cb_renderer_render_passes(self._h, passes, kernel_variant), "cb_renderer_render_passes")

    def finish(self):
        """Complete the orbits carried between launches (the read functions do this themselves)."""
        _check(lib.cb_renderer_finish(self._h), "cb_renderer_finish")

    def read_histogram(self):
        planes = self._planes()
        out = np.empty(max(planes, 1) * self.dims.w * self.dims.h, dtype=np.uint64)
        _check(lib.cb_renderer_read_histogram(self._h, out.ctypes.data), "cb_renderer_read_histogram")
        return out.reshape(planes, self.dims.h, self.dims.w) if planes else out.reshape(self.dims.h, self.dims.w)

    def read_rng_states(self):
        """True-resume checkpoint (N3): the generator states as bytes (six u32 planes of n_threads)."""
        out = np.empty(rng_state_bytes(self.n_threads), dtype=np.uint8)
        _check(lib.cb_renderer_read_rng_states(self._h, out.ctypes.data), "cb_renderer_read_rng_states")
        return out

    def write_rng_states(self, blob):
        a = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        if a.size != rng_state_bytes(self.n_threads):
            raise ValueError("generator state blob does not match n_threads")
        _check(lib.cb_renderer_write_rng_states(self._h, a.ctypes.data), "cb_renderer_write_rng_states")

    def grayscale_image(self, gamma, mode=0, plane=0):
        """Device tone map (N1) -> (big-endian u16 image [h,w] = the PGM body, max count, scale)."""
        gray = np.empty((self.dims.h, self.dims.w), dtype=">u2")
        mx, scale = C.c_uint64(), C.c_double()
        _check(
            lib.cb_renderer_grayscale_plane(self._h, int(plane), float(gamma), int(mode), gray.ctypes.data,
                                            C.byref(mx), C.byref(scale)),
            "cb_renderer_grayscale_plane",
        )
        return gray, int(mx.value), float(scale.value)

    def set_white_clip(self, percent):
        """The white clip of every image call (cb_renderer_set_white_clip): a percentage of the lit counters, 0 = off."""
        _check(lib.cb_renderer_set_white_clip(self._h, float(percent)), "cb_renderer_set_white_clip")

    @property
    def white_clip(self):
        percent = C.c_double()
        _check(lib.cb_renderer_white_clip(self._h, C.byref(percent)), "cb_renderer_white_clip")
        return float(percent.value)

    def last_white(self):
        """(white, lit, clipped) of the last image call made with a clip set (cb_renderer_last_white)."""
        white, lit, clipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib.cb_renderer_last_white(self._h, C.byref(white), C.byref(lit), C.byref(clipped)), "cb_renderer_last_white")
        return int(white.value), int(lit.value), int(clipped.value)

    def set_density_filter(self, radius, alpha=0.5, n0=1):
        """The density filter of every image call (cb_renderer_set_density_filter): "Density filter"; radius 0 = off."""
        _check(lib.cb_renderer_set_density_filter(self._h, int(radius), float(alpha), int(n0)),
               "cb_renderer_set_density_filter")

    @property
    def density_filter(self):
        """(radius, alpha, n0) as set; (0, 0.0, 0) without a filter."""
        radius, alpha, n0 = C.c_int32(), C.c_double(), C.c_uint64()
        _check(lib.cb_renderer_density_filter(self._h, C.byref(radius), C.byref(alpha), C.byref(n0)),
               "cb_renderer_density_filter")
        return int(radius.value), float(alpha.value), int(n0.value)

    def set_equalize(self, on=True):
        """Equalisation of every image call (cb_renderer_set_equalize): "Equalised image"; refused beside a white clip."""
        _check(lib.cb_renderer_set_equalize(self._h, 1 if on else 0), "cb_renderer_set_equalize")

    @property
    def equalize(self):
        return bool(lib.cb_renderer_equalize(self._h))

    def last_equalize(self):
        """(lit, keys, levels) of the last image call made equalised (cb_renderer_last_equalize)."""
        lit, keys, levels = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib.cb_renderer_last_equalize(self._h, C.byref(lit), C.byref(keys), C.byref(levels)),
               "cb_renderer_last_equalize")
        return int(lit.value), int(keys.value), int(levels.value)

    def set_local_equalize(self, tx, ty=None, clip_q=LOCAL_EQUALIZE_CLIP_Q):
        """Local equalisation of every image call (cb_renderer_set_local_equalize): "Locally equalised image", a grid of
        tx x ty tiles (ty = tx by default) and a clip in 1/256ths; tx = 0 turns it off.  Refused beside a white clip or
        equalisation."""
        tx = int(tx)
        _check(lib.cb_renderer_set_local_equalize(self._h, tx, tx if ty is None else int(ty), int(clip_q)),
               "cb_renderer_set_local_equalize")

    @property
    def local_equalize(self):
        """(tx, ty, clip_q) as set; (0, 0, 0) without."""
        tx, ty, clip_q = C.c_int32(), C.c_int32(), C.c_uint32()
        _check(lib.cb_renderer_local_equalize(self._h, C.byref(tx), C.byref(ty), C.byref(clip_q)), "cb_renderer_local_equalize")
        return int(tx.value), int(ty.value), int(clip_q.value)

    def last_local_equalize(self):
        """(lit, lit_tiles, moved) of the last image call made locally equalised (cb_renderer_last_local_equalize)."""
        lit, lit_tiles, moved = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib.cb_renderer_last_local_equalize(self._h, C.byref(lit), C.byref(lit_tiles), C.byref(moved)),
               "cb_renderer_last_local_equalize")
        return int(lit.value), int(lit_tiles.value), int(moved.value)

    def color_image(self, planes=(0, 1, 2), gamma=1.0, mode=0, compose="rgb", stretch=(2.0, 1.0), hue_shift=0.0):
        """Colour stage on the device (cb_renderer_color_image): planes[0..2] -> (big-endian u16 image [h,w,3] = the
        PPM body, levels [(black, white)] * 3)."""
        rgb = np.empty((self.dims.h, self.dims.w, 3), dtype=">u2")
        levels = np.zeros(6, dtype=np.uint16)
        idx = (C.c_int * 3)(*[int(j) for j in planes])
        params = ColorParams.make(compose, stretch, hue_shift)
        _check(
            lib.cb_renderer_color_image(self._h, idx, float(gamma), int(mode), C.byref(params), rgb.ctypes.data,
                                        levels.ctypes.data),
            "cb_renderer_color_image",
        )
        return rgb, _level_pairs(levels)

    def write_histogram(self, hist):
        a = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
        if a.size != max(self._planes(), 1) * self.dims.w * self.dims.h:
            raise ValueError("histogram size does not match the canvas")
        _check(lib.cb_renderer_write_histogram(self._h, a.ctypes.data), "cb_renderer_write_histogram")

    def read_counters(self):
        c = Counters()
        _check(lib.cb_renderer_read_counters(self._h, C.byref(c)), "cb_renderer_read_counters")
        return c

    @property
    def device_histogram(self):
        return lib.cb_renderer_device_histogram(self._h)

    def close(self):
        if self._h:
            lib.cb_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_grayscale_pixels(hist, gamma):
    """SetGrayscalePixels (cudabrot.cu:454-468) -> (u16 image [h,w] host-endian, max count, scale)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    h, w = a.shape
    gray = np.empty((h, w), dtype=np.uint16)
    mx, scale = C.c_uint64(), C.c_double()
    lib.cb_set_grayscale_pixels(a.ctypes.data, w, h, float(gamma), gray.ctypes.data, C.byref(mx), C.byref(scale))
    return gray, int(mx.value), float(scale.value)


def white_count(hist, clip):
    """The white point of an array of counters ("White clip", cb_white_count) -> (white, lit, clipped)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    white, lit, clipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib.cb_white_count(a.ctypes.data, a.size, float(clip), C.byref(white), C.byref(lit), C.byref(clipped)),
           "cb_white_count")
    return int(white.value), int(lit.value), int(clipped.value)


def set_grayscale_pixels_white(hist, gamma, clip):
    """cb_set_grayscale_pixels_white -> (u16 image [h,w] host-endian, max count, scale applied, white)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    h, w = a.shape
    gray = np.empty((h, w), dtype=np.uint16)
    mx, scale, white = C.c_uint64(), C.c_double(), C.c_uint64()
    _check(
        lib.cb_set_grayscale_pixels_white(a.ctypes.data, w, h, float(gamma), float(clip), gray.ctypes.data, C.byref(mx),
                                          C.byref(scale), C.byref(white)),
        "cb_set_grayscale_pixels_white",
    )
    return gray, int(mx.value), float(scale.value), int(white.value)


CB_EQUALIZE_KEYS = 56320  # equalised image: the number of keys


def equalize_key(count):
    """The key of a counter ("Equalised image", cb_equalize_key)."""
    return int(lib.cb_equalize_key(int(count)))


def equalize_bins(hist):
    """cb_equalize_bins over every counter of `hist` as one array -> (u64 bins [CB_EQUALIZE_KEYS], lit, max)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    bins = np.empty(CB_EQUALIZE_KEYS, dtype=np.uint64)
    lit, mx = C.c_uint64(), C.c_uint64()
    _check(lib.cb_equalize_bins(a.ctypes.data, a.size, bins.ctypes.data, C.byref(lit), C.byref(mx)), "cb_equalize_bins")
    return bins, int(lit.value), int(mx.value)


def equalize_table(bins, gamma):
    """cb_equalize_table -> (u16 table [CB_EQUALIZE_KEYS], keys, levels)."""
    b = np.ascontiguousarray(bins, dtype=np.uint64)
    assert b.shape == (CB_EQUALIZE_KEYS,)
    table = np.empty(CB_EQUALIZE_KEYS, dtype=np.uint16)
    keys, levels = C.c_uint64(), C.c_uint64()
    _check(lib.cb_equalize_table(b.ctypes.data, float(gamma), table.ctypes.data, C.byref(keys), C.byref(levels)),
           "cb_equalize_table")
    return table, int(keys.value), int(levels.value)


def set_grayscale_pixels_equalized(hist, gamma):
    """cb_set_grayscale_pixels_equalized -> (u16 image [h,w] host-endian, max count, 65535 / max, lit)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    h, w = a.shape
    gray = np.empty((h, w), dtype=np.uint16)
    mx, scale, lit = C.c_uint64(), C.c_double(), C.c_uint64()
    _check(
        lib.cb_set_grayscale_pixels_equalized(a.ctypes.data, w, h, float(gamma), gray.ctypes.data, C.byref(mx),
                                              C.byref(scale), C.byref(lit)),
        "cb_set_grayscale_pixels_equalized",
    )
    return gray, int(mx.value), float(scale.value), int(lit.value)


def equalize_bins_device(d_hist, n, stream=0):
    """cb_equalize_bins_device on caller-owned device memory (an integer pointer to n u64) -> (bins, lit, max)."""
    bins = np.empty(CB_EQUALIZE_KEYS, dtype=np.uint64)
    lit, mx = C.c_uint64(), C.c_uint64()
    _check(lib.cb_equalize_bins_device(d_hist, int(n), bins.ctypes.data, C.byref(lit), C.byref(mx), stream),
           "cb_equalize_bins_device")
    return bins, int(lit.value), int(mx.value)


def tone_map_device_equalized(d_hist, w, h, gamma, d_gray_be, stream=0):
    """cb_tone_map_device_equalized on caller-owned device memory (integer pointers) -> (max, scale, lit, keys, levels)."""
    mx, scale, lit, keys, levels = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(
        lib.cb_tone_map_device_equalized(d_hist, w, h, float(gamma), d_gray_be, C.byref(mx), C.byref(scale), C.byref(lit),
                                         C.byref(keys), C.byref(levels), stream),
        "cb_tone_map_device_equalized",
    )
    return int(mx.value), float(scale.value), int(lit.value), int(keys.value), int(levels.value)


def _planes_of(hist):
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


def local_equalize_bins(hist, tx, ty):
    """cb_local_equalize_bins over `hist` [h,w] or [planes,h,w] -> (u64 bins [ty*tx, CB_EQUALIZE_KEYS], lit, max)."""
    a = _planes_of(hist)
    planes, h, w = a.shape
    bins = np.empty((max(int(tx) * int(ty), 1), CB_EQUALIZE_KEYS), dtype=np.uint64)
    lit, mx = C.c_uint64(), C.c_uint64()
    _check(lib.cb_local_equalize_bins(a.ctypes.data, w, h, planes, int(tx), int(ty), bins.ctypes.data, C.byref(lit), C.byref(mx)),
           "cb_local_equalize_bins")
    return bins, int(lit.value), int(mx.value)


def local_equalize_clip(bins, clip_q):
    """cb_local_equalize_clip of one tile's bins -> (u64 clipped [CB_EQUALIZE_KEYS], moved)."""
    b = np.ascontiguousarray(bins, dtype=np.uint64)
    assert b.shape == (CB_EQUALIZE_KEYS,)
    clipped = np.empty(CB_EQUALIZE_KEYS, dtype=np.uint64)
    moved = C.c_uint64()
    _check(lib.cb_local_equalize_clip(b.ctypes.data, int(clip_q), clipped.ctypes.data, C.byref(moved)), "cb_local_equalize_clip")
    return clipped, int(moved.value)


def set_grayscale_pixels_local_equalized(hist, tx, ty, clip_q, gamma):
    """cb_set_grayscale_pixels_local_equalized over `hist` [h,w] or [planes,h,w] -> (u16 image in the shape of `hist`,
    host-endian, max count, 65535 / max, lit, lit_tiles, moved)."""
    a = _planes_of(hist)
    planes, h, w = a.shape
    gray = np.empty(np.shape(hist), dtype=np.uint16)
    mx, scale, lit, lit_tiles, moved = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(
        lib.cb_set_grayscale_pixels_local_equalized(a.ctypes.data, w, h, planes, int(tx), int(ty), int(clip_q), float(gamma),
                                                    gray.ctypes.data, C.byref(mx), C.byref(scale), C.byref(lit),
                                                    C.byref(lit_tiles), C.byref(moved)),
        "cb_set_grayscale_pixels_local_equalized",
    )
    return gray, int(mx.value), float(scale.value), int(lit.value), int(lit_tiles.value), int(moved.value)


def local_equalize_bins_device(d_hist, w, h, planes, tx, ty, stream=0):
    """cb_local_equalize_bins_device on caller-owned device memory (an integer pointer to planes*h*w u64) -> (bins
    [ty*tx, CB_EQUALIZE_KEYS], lit, max)."""
    bins = np.empty((int(tx) * int(ty), CB_EQUALIZE_KEYS), dtype=np.uint64)
    lit, mx = C.c_uint64(), C.c_uint64()
    _check(lib.cb_local_equalize_bins_device(d_hist, w, h, planes, int(tx), int(ty), bins.ctypes.data, C.byref(lit),
                                             C.byref(mx), stream),
           "cb_local_equalize_bins_device")
    return bins, int(lit.value), int(mx.value)


def tone_map_device_local_equalized(d_hist, w, h, planes, tx, ty, clip_q, gamma, d_gray_be, stream=0):
    """cb_tone_map_device_local_equalized on caller-owned device memory (integer pointers) -> (max, scale, lit, lit_tiles,
    moved)."""
    mx, scale, lit, lit_tiles, moved = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(
        lib.cb_tone_map_device_local_equalized(d_hist, w, h, planes, int(tx), int(ty), int(clip_q), float(gamma), d_gray_be,
                                               C.byref(mx), C.byref(scale), C.byref(lit), C.byref(lit_tiles),
                                               C.byref(moved), stream),
        "cb_tone_map_device_local_equalized",
    )
    return int(mx.value), float(scale.value), int(lit.value), int(lit_tiles.value), int(moved.value)


def density_thresholds(radius, alpha=0.5, n0=1):
    """T[0 .. R] of the density filter ("Density filter", cb_density_thresholds) as a list of ints."""
    radius = int(radius)
    table = (C.c_uint64 * (max(radius, 0) + 1))()
    _check(lib.cb_density_thresholds(radius, float(alpha), int(n0), table), "cb_density_thresholds")
    return [int(t) for t in table]


def _density_table(thresholds):
    return (C.c_uint64 * len(thresholds))(*[int(t) for t in thresholds])


def density_filter(hist, thresholds, group=1):
    """cb_density_filter on a host array [h, w] or [planes, h, w] -> u64 array of the same shape, 8 fraction bits;
    thresholds = T[0 .. R] (density_thresholds)."""
    a = np.ascontiguousarray(hist, dtype=np.uint64)
    planes, h, w = (1,) + a.shape if a.ndim == 2 else a.shape
    out = np.zeros_like(a)
    _check(lib.cb_density_filter(a.ctypes.data, w, h, planes, int(group), len(thresholds) - 1, _density_table(thresholds),
                                 out.ctypes.data), "cb_density_filter")
    return out


def density_filter_device(d_hist, w, h, planes, group, thresholds, d_out, stream=0):
    """cb_density_filter_device on caller-owned device memory (integer pointers to planes * h * w u64 each)."""
    _check(lib.cb_density_filter_device(d_hist, int(w), int(h), int(planes), int(group), len(thresholds) - 1,
                                        _density_table(thresholds), d_out, stream), "cb_density_filter_device")


def white_count_device(d_hist, n, clip, stream=0):
    """cb_white_count_device on caller-owned device memory (an integer pointer to n u64) -> (white, lit, clipped)."""
    white, lit, clipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib.cb_white_count_device(d_hist, int(n), float(clip), C.byref(white), C.byref(lit), C.byref(clipped), stream),
           "cb_white_count_device")
    return int(white.value), int(lit.value), int(clipped.value)


def tone_map_device_white(d_hist, w, h, gamma, clip, d_gray_be, mode=0, stream=0):
    """cb_tone_map_device_white on caller-owned device memory (integer pointers) -> (max count, scale applied, white)."""
    mx, scale, white = C.c_uint64(), C.c_double(), C.c_uint64()
    _check(
        lib.cb_tone_map_device_white(d_hist, w, h, float(gamma), int(mode), float(clip), d_gray_be, C.byref(mx),
                                     C.byref(scale), C.byref(white), stream),
        "cb_tone_map_device_white",
    )
    return int(mx.value), float(scale.value), int(white.value)


def draw_buddhabrot_channels(dims, d_hist, windows, d_states, n_threads, samples_per_thread, d_counters=0,
                             kernel_variant=CB_KERNEL_DEFAULT, stream=0, d_workspace=0, workspace_bytes=0, d_carry=0):
    """Fused multi-channel launch (N2): windows = [(max_iter, min_iter), ...]; d_hist = len(windows) planes."""
    arr = (IterationControl * len(windows))(*[IterationControl(int(m), int(c)) for m, c in windows])
    _check(
        lib.cb_draw_buddhabrot_channels(C.byref(dims), d_hist, arr, len(windows), d_states, n_threads,
                                        samples_per_thread, d_counters, kernel_variant, d_workspace, workspace_bytes,
                                        d_carry, stream),
        "cb_draw_buddhabrot_channels",
    )


def flush_scatter_channels(dims, d_hist, n_channels, n_threads, d_workspace, workspace_bytes, stream=0):
    _check(
        lib.cb_flush_scatter_channels(C.byref(dims), d_hist, n_channels, n_threads, d_workspace, workspace_bytes, stream),
        "cb_flush_scatter_channels",
    )


def renderers_reduce(renderers):
    """renderers[0] += renderers[1:] (cb_renderers_reduce: RCCL across devices, an add kernel on one device)."""
    arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
    _check(lib.cb_renderers_reduce(arr, len(renderers)), "cb_renderers_reduce")


def tone_value(count, max_count, gamma):
    """One pixel of SetGrayscalePixels (cudabrot.cu:443-449,462-466)."""
    return int(lib.cb_tone_value(int(count), int(max_count), float(gamma)))


def tone_map_device(d_hist, w, h, gamma, d_gray_be, mode=0, stream=0):
    """cb_tone_map_device on caller-owned device memory (integer pointers) -> (max count, scale)."""
    mx, scale = C.c_uint64(), C.c_double()
    _check(
        lib.cb_tone_map_device(d_hist, w, h, float(gamma), int(mode), d_gray_be, C.byref(mx), C.byref(scale), stream),
        "cb_tone_map_device",
    )
    return int(mx.value), float(scale.value)


def save_image(path, gray):
    """SaveImage (cudabrot.cu:548-577); ``gray`` is copied (the C call byte-swaps in place)."""
    g = np.array(gray, dtype=np.uint16, order="C")
    h, w = g.shape
    return int(lib.cb_save_image(os.fsencode(path), g.ctypes.data, w, h))


def _level_pairs(levels):
    return [(int(levels[2 * j]), int(levels[2 * j + 1])) for j in range(3)]


def compose_color(grays, compose="rgb", stretch=(2.0, 1.0), hue_shift=0.0):
    """Colour stage on the host (cb_compose_color): three u16 images [h,w] (the values of the PGMs) ->
    (big-endian u16 image [h,w,3] = the PPM body, levels [(black, white)] * 3)."""
    planes = [np.ascontiguousarray(g, dtype=np.uint16) for g in grays]
    if len(planes) != 3 or any(g.ndim != 2 or g.shape != planes[0].shape for g in planes):
        raise ValueError("compose_color wants three images of one shape")
    h, w = planes[0].shape
    rgb = np.empty((h, w, 3), dtype=">u2")
    levels = np.zeros(6, dtype=np.uint16)
    ptrs = (C.c_void_p * 3)(*[g.ctypes.data for g in planes])
    params = ColorParams.make(compose, stretch, hue_shift)
    _check(lib.cb_compose_color(ptrs, w, h, C.byref(params), rgb.ctypes.data, levels.ctypes.data), "cb_compose_color")
    return rgb, _level_pairs(levels)


def compose_color_device(d_hists, w, h, gamma, d_rgb_be, mode=0, compose="rgb", stretch=(2.0, 1.0), hue_shift=0.0,
                         stream=0):
    """cb_compose_color_device on caller-owned device memory (integer pointers: three histograms of w*h u64, the
    3*w*h u16 of the output) -> levels [(black, white)] * 3."""
    levels = np.zeros(6, dtype=np.uint16)
    ptrs = (C.c_void_p * 3)(*[int(p) for p in d_hists])
    params = ColorParams.make(compose, stretch, hue_shift)
    _check(
        lib.cb_compose_color_device(ptrs, w, h, float(gamma), int(mode), C.byref(params), d_rgb_be, levels.ctypes.data,
                                    stream),
        "cb_compose_color_device",
    )
    return _level_pairs(levels)


def save_ppm(path, rgb):
    """Binary 16-bit PPM of an image [h,w,3] (cb_save_ppm_be) -> 0, or 1/2/3 as save_image."""
    a = np.ascontiguousarray(rgb, dtype=">u2")
    h, w, _ = a.shape
    return int(lib.cb_save_ppm_be(os.fsencode(path), a.ctypes.data, w, h))
