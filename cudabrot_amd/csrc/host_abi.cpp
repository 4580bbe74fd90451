// host_abi.cpp -- the entry points of the C ABI that are plain host arithmetic (no device call), kept apart from
// capi.hip so that the sanitized CPU build (tests/asan) links them without the HIP runtime.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cudabrot_amd.h"

extern "C" {

int cb_recompute_pixel_deltas(cb_fractal_dimensions *dims, const char **msg) {
  const char *m = nullptr;
  if (dims->w <= 0) {
    m = "Output width must be positive.";
  } else if (dims->h <= 0) {
    m = "Output height must be positive.";
  } else if (dims->max_real <= dims->min_real) {
    m = "Maximum real value must be greater than minimum real value.";
  } else if (dims->max_imag <= dims->min_imag) {
    // (sic) the reference's wording, cudabrot.cu:520-521
    m = "Minimum imaginary value must be greater than maximum imaginary value.";
  }
  if (m) {
    if (msg) *msg = m;
    return 0;
  }
  dims->delta_imag = (dims->max_imag - dims->min_imag) / ((double) dims->h);
  dims->delta_real = (dims->max_real - dims->min_real) / ((double) dims->w);
  return 1;
}

// The one gate of the test / tuning knobs ("Diagnostics and test knobs"): a CUDABROT_AMD_* variable is
// read only when CUDABROT_AMD_DEBUG=1 is set as well, so a stray variable in a user's environment cannot change
// the path the product takes.
const char *cb_debug_knob(const char *name) {
  const char *gate = getenv("CUDABROT_AMD_DEBUG");
  if (!gate || strcmp(gate, "1") != 0 || !name) return nullptr;
  return getenv(name);
}

size_t cb_rng_state_bytes(uint32_t n_threads) { return (size_t) n_threads * 6u * sizeof(uint32_t); }

// ---- focused render: the host side of the cell list (include/cudabrot_amd.h, "Focused render") ----------------------

size_t cb_focus_mask_bytes(int level) {
  if (level < CB_FOCUS_MIN_LEVEL || level > CB_FOCUS_MAX_LEVEL) return 0;
  const size_t n = (size_t) 4 << level;
  return n * n / 8;  // n is a multiple of 64
}

// The mask dilated by `dilate` cells in the Chebyshev metric = a box of side 2 d + 1 = a horizontal pass (is any cell
// of [col - d, col + d] set?) followed by a vertical one over its result.  Each is a sliding count, so the cost is
// O(n^2) whatever d; the vertical pass keeps one count per column and walks whole rows.  Not hot: 16 Mi cells at the
// largest level.
int cb_focus_cells(int level, const uint32_t *mask_host, int dilate, uint32_t *cells_out, uint32_t *n_cells) {
  const int kInvalidValue = 1;  // hipErrorInvalidValue
  if (level < CB_FOCUS_MIN_LEVEL || level > CB_FOCUS_MAX_LEVEL || !mask_host || !n_cells || dilate < 0) {
    return kInvalidValue;
  }
  const long n = 4L << level;
  const long d = dilate < n ? dilate : n;  // beyond the grid's side every larger d gives the same
  unsigned char *wide = (unsigned char *) malloc((size_t) n * (size_t) n);  // after the horizontal pass
  uint32_t *count = (uint32_t *) calloc((size_t) n, sizeof(uint32_t));      // set cells of a column inside the window
  if (!wide || !count) {
    free(wide);
    free(count);
    return 2;  // hipErrorOutOfMemory
  }
  for (long row = 0; row < n; ++row) {
    const size_t base = (size_t) row * (size_t) n;
    auto bit = [&](long col) { return (mask_host[(base + (size_t) col) >> 5] >> ((base + (size_t) col) & 31u)) & 1u; };
    uint32_t inside = 0;  // set cells of [col - d, col + d], clipped
    for (long col = 0; col < d && col < n; ++col) inside += bit(col);
    for (long col = 0; col < n; ++col) {
      if (col + d < n) inside += bit(col + d);
      if (col - d - 1 >= 0) inside -= bit(col - d - 1);
      wide[base + (size_t) col] = inside != 0;
    }
  }
  uint32_t found = 0;
  for (long row = 0; row < d && row < n; ++row) {
    for (long col = 0; col < n; ++col) count[col] += wide[(size_t) row * (size_t) n + (size_t) col];
  }
  for (long row = 0; row < n; ++row) {
    const unsigned char *enter = row + d < n ? wide + (size_t) (row + d) * (size_t) n : nullptr;
    const unsigned char *leave = row - d - 1 >= 0 ? wide + (size_t) (row - d - 1) * (size_t) n : nullptr;
    for (long col = 0; col < n; ++col) {
      if (enter) count[col] += enter[col];
      if (leave) count[col] -= leave[col];
      if (count[col] != 0) {
        if (cells_out) cells_out[found] = (uint32_t) (row * n + col);
        found++;
      }
    }
  }
  free(wide);
  free(count);
  *n_cells = found;
  return 0;
}

// ---- palette render: the table of a list of colour stops (include/cudabrot_amd.h, "Palette render") ----------------

int cb_palette_from_stops(const cb_palette_stop *stops, int n_stops, uint32_t *lut_out, uint32_t n_entries) {
  const int kInvalidValue = 1;  // hipErrorInvalidValue
  if (!stops || !lut_out || n_stops < 1 || n_stops > CB_PALETTE_MAX_STOPS || n_entries < 1u ||
      n_entries > (uint32_t) CB_PALETTE_MAX_ENTRIES) {
    return kInvalidValue;
  }
  for (int j = 0; j < n_stops; ++j) {
    const cb_palette_stop &s = stops[j];
    if (s.k < 0 || (j > 0 && s.k <= stops[j - 1].k) || s.r < 0 || s.r > 255 || s.g < 0 || s.g > 255 || s.b < 0 || s.b > 255) {
      return kInvalidValue;
    }
  }
  int above = 0;  // the first stop with k_stop > k
  for (uint32_t k = 0; k < n_entries; ++k) {
    while (above < n_stops && (uint64_t) stops[above].k <= k) above++;
    const cb_palette_stop &a = stops[above > 0 ? above - 1 : 0];
    const cb_palette_stop &b = stops[above < n_stops ? above : n_stops - 1];
    uint32_t rgb[3];
    const int va[3] = {a.r, a.g, a.b}, vb[3] = {b.r, b.g, b.b};
    for (int j = 0; j < 3; ++j) {
      if (above == 0 || above == n_stops) {  // at or before the first stop, at or after the last
        rgb[j] = (uint32_t) (above == 0 ? va[j] : vb[j]);
      } else {
        const uint64_t span = (uint64_t) (b.k - a.k);
        rgb[j] = (uint32_t) (((uint64_t) va[j] * ((uint64_t) b.k - k) + (uint64_t) vb[j] * (k - (uint64_t) a.k) + span / 2) / span);
      }
    }
    lut_out[k] = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
  }
  return 0;
}

// ---- frames render: one rotation, and the matrices of a sweep (include/cudabrot_amd.h, "Frames render") -------------

// The one place a projection is rotated: the `--rotate` flag (cli_args.cpp) and cb_frames_from_sweep both come here.
int cb_rotate_projection(double p[8], int axis_x, int axis_y, double degrees) {
  const int kInvalidValue = 1;  // hipErrorInvalidValue
  if (!p || axis_x < 0 || axis_x > 3 || axis_y < 0 || axis_y > 3 || axis_x == axis_y || !isfinite(degrees)) {
    return kInvalidValue;
  }
  // An integer multiple of 90 degrees uses exact 0 and +-1 (a permutation of the two columns with signs); otherwise the
  // host's cos and sin.
  double co, si;
  const double quarters = degrees / 90.0;
  if (quarters == floor(quarters)) {
    const int q = (int) fmod(fmod(quarters, 4.0) + 4.0, 4.0);
    co = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
    si = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
  } else {
    const double radians = degrees * (M_PI / 180.0);
    co = cos(radians);
    si = sin(radians);
  }
  for (int row = 0; row < 2; ++row) {
    const double a = p[4 * row + axis_x], b = p[4 * row + axis_y];
    p[4 * row + axis_x] = (a * co - b * si) + 0.0;  // (+ 0.0: an exact zero is +0)
    p[4 * row + axis_y] = (a * si + b * co) + 0.0;
  }
  return 0;
}

int cb_frames_from_sweep(const double base[8], int axis_x, int axis_y, double deg0, double deg1, int n_frames, double *out,
                         double *angles_out) {
  const int kInvalidValue = 1;  // hipErrorInvalidValue
  if (!base || !out || axis_x < 0 || axis_x > 3 || axis_y < 0 || axis_y > 3 || axis_x == axis_y || !isfinite(deg0) ||
      !isfinite(deg1) || n_frames < 1 || n_frames > CB_FRAMES_MAX) {
    return kInvalidValue;
  }
  for (int j = 0; j < 8; ++j) {
    if (!isfinite(base[j])) return kInvalidValue;
  }
  // (deg1 - deg0 of two finite angles can overflow: every a_f is looked at before anything is written)
  for (int f = 0; f < n_frames; ++f) {
    if (!isfinite(deg0 + ((deg1 - deg0) * (double) f) / (double) n_frames)) return kInvalidValue;
  }
  for (int f = 0; f < n_frames; ++f) {
    const double a_f = deg0 + ((deg1 - deg0) * (double) f) / (double) n_frames;
    double *p = out + 8 * (size_t) f;
    memcpy(p, base, 8 * sizeof(double));  // every frame from the base, never from the frame before
    (void) cb_rotate_projection(p, axis_x, axis_y, a_f);
    if (angles_out) angles_out[f] = a_f;
  }
  return 0;
}

}  // extern "C"
