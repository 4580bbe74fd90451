// capi.hip -- implementation of include/cudabrot_amd.h (the C ABI).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "color_math.h"
#include "kernels.h"

namespace {

#define CB_TRY(expr)                       \
  do {                                     \
    hipError_t cb_e_ = (expr);             \
    if (cb_e_ != hipSuccess) return (int) cb_e_; \
  } while (0)

// The flags a kernel variant may carry beside its base (CB_KERNEL_DEFAULT ... CB_KERNEL_FULL_ITERATE).
constexpr int kVariantFlags = CB_KERNEL_FLAG_BURNING_SHIP | CB_KERNEL_FLAG_DRAIN | CB_KERNEL_FLAG_ANTI;

// One copy of the jump matrices per device, created on first use and kept for the process lifetime.
std::mutex g_matrix_mutex;
const uint32_t *g_matrices[64] = {nullptr};

int device_matrices(const uint32_t **out) {
  int dev = 0;
  CB_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return (int) hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(g_matrix_mutex);
  if (!g_matrices[dev]) {
    std::vector<uint32_t> host((size_t) cb::kSeqJumpMatrices * cb::kMatrixWords);
    cb::build_sequence_jump_matrices(host.data());
    uint32_t *d = nullptr;
    CB_TRY(hipMalloc(&d, host.size() * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(d, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void) hipFree(d);
      return (int) e;
    }
    g_matrices[dev] = d;
  }
  *out = g_matrices[dev];
  return 0;
}

// ---- the interior map: data that decides what the kernels compute --------------------------------------------------
//
// One bit per cell of side 2^-level of the c-plane: every sample of a marked cell provably never escapes (made and PROVEN
// on the CPU by tools/interior_map.c; DrawArgs::interior_map).  It is EMBEDDED in this library and in the binary (maps.S:
// .incbin of the file `make` unpacks and whose sha256 it checks against the digest kept in the tree) -- there is no file
// to find, lose or swap at run time.  One copy per device, made on first use.  CUDABROT_AMD_INTERIOR_MAP=<file> (a test
// knob, behind CUDABROT_AMD_DEBUG=1) takes another map of the same format -- header, level and EXACT length are checked;
// anything else is an error, never a fallback.
extern "C" {
extern const unsigned char cb_embedded_interior_map[], cb_embedded_interior_map_end[];
}

enum MapKind { kMapInterior = 0, kMapKinds };
struct DeviceMap {
  const unsigned char *d_bytes;
  uint32_t level, cols, rows;
};
std::mutex g_map_mutex;
DeviceMap g_maps[64][kMapKinds];
int g_map_state[64][kMapKinds] = {{0}};  // 0: not tried, 1: there, -1: failed (reported once)
std::atomic<int> g_interior_level{0};    // cb_debug_interior_map_level: the level of the map the last launch used (0: none)

// header: magic, level, columns, rows (u32 each); then the payload, whose length the header implies
bool parse_map(MapKind, const unsigned char *bytes, size_t n, DeviceMap *out, size_t *payload) {
  if (n < 16) return false;
  uint32_t h[4];
  memcpy(h, bytes, 16);
  const uint32_t level = h[1];
  if (h[0] != 0x4d494243u /* "CBIM" */ || level < 8u || level > 15u || h[2] != (5u << level) / 2u ||
      h[3] != (5u << level) / 4u) {  // 2.5 and 1.25 * 2^level
    return false;
  }
  *payload = ((size_t) h[2] * h[3] + 7) / 8;
  if (n != 16 + *payload) return false;  // not a byte more or less
  *out = DeviceMap{nullptr, level, h[2], h[3]};
  return true;
}

const DeviceMap *device_map(MapKind kind) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(g_map_mutex);
  if (g_map_state[dev][kind] == 0) {
    g_map_state[dev][kind] = -1;
    const unsigned char *bytes = cb_embedded_interior_map;
    size_t n = (size_t) (cb_embedded_interior_map_end - cb_embedded_interior_map);
    std::vector<unsigned char> file;
    const char *knob = cb_debug_knob("CUDABROT_AMD_INTERIOR_MAP");
    if (knob) {  // (a test knob: another map)
      FILE *f = fopen(knob, "rb");
      if (f) {
        unsigned char buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
      }
      bytes = file.data();
      n = file.size();
    }
    DeviceMap m;
    size_t payload = 0;
    if (!parse_map(kind, bytes, n, &m, &payload)) {
      fprintf(stderr, "cudabrot_amd: %s is not a map of the kind it stands for (header, level or length): refused\n",
              knob ? knob : "the embedded map");
      return nullptr;
    }
    const unsigned char *src = bytes + 16;
    unsigned char *d = nullptr;
    if (hipMalloc(&d, payload) != hipSuccess) return nullptr;
    if (hipMemcpy(d, src, payload, hipMemcpyHostToDevice) != hipSuccess) {
      (void) hipFree(d);
      return nullptr;
    }
    m.d_bytes = d;
    g_maps[dev][kind] = m;
    g_map_state[dev][kind] = 1;
  }
  return g_map_state[dev][kind] == 1 ? &g_maps[dev][kind] : nullptr;
}

// The interior map for a launch of the wave-scheduled kernels (their MID stage in its one-piece form looks samples up;
// the lock-step kernel and the other forms ignore it): where orbits may be retired early at all -- not the Burning
// Ship, not the full-iterate variants, not the anti-Buddhabrot, which plots exactly the samples the map retires
// (CUDABROT_AMD_NO_INTERIOR_MAP=1, a test knob: never).  0, or an error: a map that should be there and is not is never
// passed over in silence.
bool wants_interior_map(int kernel_variant) {
  const int base_variant = kernel_variant & ~kVariantFlags;
  return !((kernel_variant & (CB_KERNEL_FLAG_BURNING_SHIP | CB_KERNEL_FLAG_ANTI)) != 0 ||
           base_variant == CB_KERNEL_FULL_ITERATE || base_variant == CB_KERNEL_SIMPLE ||
           cb_debug_knob("CUDABROT_AMD_TIMED_FULL") != nullptr || cb_debug_knob("CUDABROT_AMD_NO_INTERIOR_MAP") != nullptr);
}
int attach_interior_map(cb::DrawArgs &a, int kernel_variant) {
  g_interior_level.store(0, std::memory_order_relaxed);
  if (!wants_interior_map(kernel_variant)) return 0;
  const DeviceMap *m = device_map(kMapInterior);
  if (!m) return (int) hipErrorInvalidValue;
  a.interior_map = m->d_bytes;
  a.interior_shift = m->level - 1u;
  a.interior_cols = m->cols;
  a.interior_rows = m->rows;
  g_interior_level.store((int) m->level, std::memory_order_relaxed);
  return 0;
}

// x / delta == x * (1 / delta) bit for bit iff delta is a (normal) power of two.
bool exact_reciprocal(double delta, double *inv) {
  int e = 0;
  if (!(delta > 0.0) || !isfinite(delta)) return false;
  if (frexp(delta, &e) != 0.5) return false;
  const double r = 1.0 / delta;
  if (!isfinite(r) || r == 0.0 || fpclassify(delta) != FP_NORMAL || fpclassify(r) != FP_NORMAL) {
    return false;
  }
  *inv = r;
  return true;
}

// Diagnostic only: which draw kernel the last cb_draw_buddhabrot* call of this process launched (cb_debug_last_draw_kernel).
std::atomic<int> g_last_draw_kernel{0};

// Diagnostic only (CUDABROT_AMD_WAVE_DUMP=<file> with the timed kernel variant): per-wave records of
// the last launch, see DrawArgs::wave_dump.
unsigned long long *g_wave_dump = nullptr;

cb::DrawArgs make_args(const cb_fractal_dimensions *dims, const cb_iteration_control *it,
                       cb_pixel *d_hist, void *d_states, uint32_t n_threads,
                       uint32_t samples_per_thread, cb_counters *d_counters, void *d_workspace,
                       size_t workspace_bytes, void *d_carry, int n_channels = 0) {
  cb::DrawArgs a;
  memset(&a, 0, sizeof(a));
  a.min_real = dims->min_real;
  a.min_imag = dims->min_imag;
  a.delta_real = dims->delta_real;
  a.delta_imag = dims->delta_imag;
  a.inv_delta_real = 0.0;
  a.inv_delta_imag = 0.0;
  a.pow2_real = exact_reciprocal(dims->delta_real, &a.inv_delta_real) ? 1 : 0;
  a.pow2_imag = exact_reciprocal(dims->delta_imag, &a.inv_delta_imag) ? 1 : 0;
  a.rcp_delta_real = 1.0 / dims->delta_real;  // only ever an estimate: any value (inf, nan) is safe
  a.rcp_delta_imag = 1.0 / dims->delta_imag;
  a.replay_min2_real = dims->min_real + dims->min_real;
  a.replay_min2_imag = dims->min_imag + dims->min_imag;
  if (a.pow2_real && a.pow2_imag) {
    a.replay_scale_real = 0.5 * a.inv_delta_real;
    a.replay_scale_imag = 0.5 * a.inv_delta_imag;
    a.replay_offset_real = -(dims->min_real * a.inv_delta_real);
    a.replay_offset_imag = -(dims->min_imag * a.inv_delta_imag);
  } else {
    a.replay_scale_real = dims->delta_real;
    a.replay_scale_imag = dims->delta_imag;
    a.replay_offset_real = dims->min_real;
    a.replay_offset_imag = dims->min_imag;
  }
  a.w = dims->w;
  a.h = dims->h;
  a.replay_bound_w = (double) dims->w;
  a.replay_bound_h = (double) dims->h;
  a.max_iter = it->max_escape_iterations;
  a.min_iter = it->min_escape_iterations;
  cb::plan_stages(a.max_iter, a.min_iter, &a.head_steps, &a.mid_steps);
  {
    const int long_steps = a.max_iter - (a.head_steps + a.mid_steps);
    a.long_steps = long_steps > 0 ? (uint32_t) long_steps : 0u;
    a.tail_steps = a.long_steps % (uint32_t) cb::kChunk;
    a.tail_value = a.tail_steps ? a.tail_steps : ~0u;
    a.accept_rem = a.max_iter - a.min_iter;
    a.fast_mid = (a.min_iter >= a.head_steps + a.mid_steps && long_steps > 0) ? 1 : 0;
    a.long_start = a.head_steps + a.mid_steps;
    a.tail_start = a.long_start + (int) (a.long_steps - a.tail_steps);
    a.sparse_long = (long_steps > 0 && a.min_iter <= a.long_start && cb_debug_knob("CUDABROT_AMD_DENSE_TESTS") == nullptr) ? 1 : 0;
    a.sparse_threshold = 16.0 - 0x1p-10;
    if (const char *e = cb_debug_knob("CUDABROT_AMD_SPARSE_THRESHOLD")) {  // test knob: only ever lower
      const double v = atof(e);
      if (v > 0.0 && v < a.sparse_threshold) a.sparse_threshold = v;
    }
  }
  a.n_threads = n_threads;
  a.samples_per_thread = samples_per_thread;
  a.hist = reinterpret_cast<unsigned long long *>(d_hist);
  a.states = reinterpret_cast<uint32_t *>(d_states);
  a.counters = d_counters;
  a.bin = cb::make_bin_layout(d_workspace, workspace_bytes, dims->w, dims->h,
                              cb::draw_wave_count(n_threads), n_channels);
  a.wave_dump = g_wave_dump;
  a.check_periodic = 1;
  a.carry = reinterpret_cast<unsigned long long *>(d_carry);
  a.drain = (d_carry != nullptr && samples_per_thread == 0) ? 1 : 0;
  return a;
}

// A draw call that launches nothing (no samples and nothing to drain) must still leave the workspace in the
// state cb_flush_scatter expects -- an empty stream -- or the flush would re-add the previous launch's stream
// (or read the counts of a workspace no kernel has written yet).
int empty_stream_if_nothing_launches(const cb::DrawArgs &a, hipStream_t stream) {
  const bool launches = a.n_threads != 0 && (a.samples_per_thread != 0 || (a.carry != nullptr && a.drain != 0));
  if (launches || !a.bin.enabled) return 0;
  return (int) hipMemsetAsync(a.bin.wave_count, 0, (size_t) a.bin.n_waves * sizeof(uint32_t), stream);
}

// Stream entries a launch is expected to produce: visited in-canvas points per sample are 0.4 (max_iter
// 100) to 1.7 (max_iter 20000) on the full canvas; anything beyond the estimate falls back to atomics.
constexpr double kEntriesPerSample = 2.5;
// Passes fused into one launch by cb_renderer.  A launch has fixed costs (the scatter's table kernels, the seams
// of the pipeline, the spread of the waves' end times): 128 instead of 64 is + 6 % on the reference's default
// canvas, + 7 % at max_iter 2000, + 2.5 % at 20000 (4096^2), + 0.5 % at 20000^2; 256 would not fit the stream's
// 32-bit entry indices.  Costs workspace: 2 x 23.7 GiB at 4096^2.
constexpr uint32_t kRendererPassesPerLaunch = 128;

// What a render is: the normal one (of a renderer: its n_channels windows fused, if any), the focused one, or a plotted one
// (draw_plot.hip and its kin: direct atomics, no deferred scatter, no carry) named by its sink -- one plane, the palette's
// three, the depth's slices, the depth palette's three, the frames, the Phoenix step's one, the bounded orbits' one, the
// period palette's three, and the aimed kinds: the projected and the bounded render drawn from a cell list (draw_aim.hip).
// Whether c is sampled or fixed (Plotted::julia) is the source beside it.  What varies with the
// kind is kind_row and draw_plotted's switch.
enum Kind { kNormal = 0, kFocus, kPlot, kPalette, kDepth, kDepthPalette, kFrames, kPhoenix, kBounded, kPeriodPalette,
            kAimed, kAimedBounded };
bool is_plotted(Kind k) { return k != kNormal && k != kFocus; }

// What every draw launch is given: the public entry points fill it from their arguments, a renderer from itself and the
// passes asked for.
struct Launch {
  const cb_fractal_dimensions *dims;
  cb_pixel *d_hist;
  const cb_iteration_control *iterations;
  void *d_states;
  uint32_t n_threads, samples_per_thread;
  cb_counters *d_counters;
  int kernel_variant;
  void *stream;
};

// The cell list of a focused or an aimed render (level 0, no cells: the uniform source), and the step bits of the kernel
// variant it was probed with -- the Burning Ship's flag alone for a focus, kStepBits for an aim; a renderer's launch with
// other bits is refused.  The renderer that keeps one owns d_cells; an entry point only lends its caller's.
struct CellList {
  int level;
  uint32_t *d_cells;
  uint32_t n_cells;
  int step_bits;
};

// What a plotted launch adds; a renderer keeps one as what it is (cb_renderer::what), and then owns the device memory.
struct Plotted {
  Kind kind;
  double projection[8];  // the matrix P[2][4] (kFrames: kept for cb_renderer_projection, the launch takes `d_frames`)
  bool julia;            // c is julia_c and the sample is z_0
  double julia_c[2];
  const uint32_t *d_lut;  // kPalette: n_entries = max_iter entries; kDepthPalette: n_entries = depth.slices entries;
                          // kPeriodPalette: n_entries = the largest period + 1
  uint32_t n_entries;
  cb_depth depth;          // kDepth, kDepthPalette
  const double *d_frames;  // kFrames: n_frames x 8 doubles
  int n_frames;
  double phoenix_p[2];  // kPhoenix
  double period_eps;    // kPeriodPalette
  CellList cells;       // kAimed, kAimedBounded; of a renderer: kFocus too
};

}  // namespace

struct cb_renderer {
  int device;
  cb_fractal_dimensions dims;
  cb_iteration_control iterations;
  uint32_t n_threads;
  cb_pixel *d_hist;
  uint32_t *d_states;
  cb_counters *d_counters;
  // Scatter workspaces, allocated on first use.  Two of them, so that the flush of launch n (on
  // flush_stream) overlaps the draw kernel of launch n+1 (on stream): the flush is HBM/LDS work, the
  // draw kernel is fp64 work.
  void *d_workspace[2];
  size_t workspace_bytes;
  int workspace_tried;
  int next_workspace;
  bool flush_pending[2];
  hipEvent_t draw_done[2], flush_done[2];
  hipStream_t stream, flush_stream;
  // In-flight work carried from launch to launch (cb_draw_buddhabrot's d_carry); drained lazily by
  // finish() before anything reads the histogram or the counters.
  void *d_carry;
  bool carry_pending;
  int carry_variant;
  // fused multi-channel render: n_channels > 0 windows, d_hist holds that many planes; a count of the normal kind only
  int n_channels;
  cb_iteration_control windows[CB_MAX_CHANNELS];
  // the level of the interior map this renderer's last launch used (0: none) -- its own record: the process-wide
  // cb_debug_interior_map_level is whichever rank's launch came last
  int interior_level;
  // what the generators were made from (cb_renderer_set_focus probes on fresh ones) and whether a pass was rendered
  uint64_t seed, first_subsequence;
  bool rendered;
  // What the renderer is, and for a plotted kind what its launches add: the setters (`admits`) are the only writers.  d_hist
  // has kind_row(what).planes planes, or n_channels.
  Plotted what;
  std::vector<double> *frames;  // kFrames: what.d_frames on the host (cb_renderer_frames)
  // The white clip ("White clip" of include/cudabrot_amd.h): an output setting the image calls read, 0 = off.  No launch,
  // histogram or generator knows of it.
  double white_clip;
  // The density filter ("Density filter" of include/cudabrot_amd.h): an output setting too, radius 0 = off, with the
  // table cb_density_thresholds made of it.
  int density_radius;
  double density_alpha;
  uint64_t density_n0;
  uint64_t density_thresholds[CB_DENSITY_MAX_RADIUS + 1];
  // Equalisation ("Equalised image" of include/cudabrot_amd.h): an output setting as well, never on beside a white clip.
  bool equalize;
  // Local equalisation ("Locally equalised image" of include/cudabrot_amd.h): an output setting too, tiles_x = 0 = off,
  // never on beside a white clip or the equalisation above.
  int local_tiles_x, local_tiles_y;
  uint32_t local_clip_q;
  // What the last image call found under the exposure set now (cb_renderer_last_white, cb_renderer_last_equalize,
  // cb_renderer_last_local_equalize): the setters clear it.
  cb::Exposed last_exposed;
};

namespace {

enum Image { kImageSingle, kImageStacked, kImageRgb };

// What varies with a render's kind beside the launch itself (draw_plotted's switch): the planes of its histogram, what its
// image call makes of them (one gray plane; all planes one above the other, gray; three planes as R, G, B), and whether its
// launches take a bare base variant only -- CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, no flag bit: the step is the render's.
struct KindRow {
  size_t planes;
  Image image;
  bool bare_variant;
};
KindRow kind_row(const Plotted &p) {
  switch (p.kind) {
    case kNormal: return {1, kImageSingle, false};  // (a channel renderer: n_channels planes, renderer_planes)
    case kFocus: return {1, kImageSingle, false};
    case kPlot: return {1, kImageSingle, false};
    case kPalette: return {3, kImageRgb, false};
    case kDepth: return {(size_t) p.depth.slices, kImageStacked, false};
    case kDepthPalette: return {3, kImageRgb, false};
    case kFrames: return {(size_t) p.n_frames, kImageStacked, false};
    case kPhoenix: return {1, kImageSingle, true};
    case kBounded: return {1, kImageSingle, false};
    case kPeriodPalette: return {3, kImageRgb, false};
    case kAimed: return {1, kImageSingle, false};
    case kAimedBounded: return {1, kImageSingle, false};
  }
  return {0, kImageSingle, false};  // (no kind)
}

size_t renderer_planes(const cb_renderer *r) { return r->n_channels ? (size_t) r->n_channels : kind_row(r->what).planes; }

bool variant_ok(const Plotted &p, int kernel_variant) {
  return !kind_row(p).bare_variant || kernel_variant == CB_KERNEL_DEFAULT || kernel_variant == CB_KERNEL_SIMPLE;
}

// May the renderer become `want`?  The one rule of every setter: only before the first pass; a channel renderer, a focused
// one and one with a sink stay what they are; a plain one takes a focus, a projection (with or without a fixed c) or a
// palette, the bounded or the period-palette sink, which bring the identity projection; a projected or Julia one without a
// sink takes any sink; an aim (kAimed) is taken by a plain one, which gains the identity projection, and by a projected or
// Julia one without a sink, and a bounded one takes the bounded aim (kAimedBounded); an aimed one takes nothing.
bool admits(const cb_renderer *r, Kind want) {
  if (!r || r->rendered || r->n_channels > 0) return false;
  switch (r->what.kind) {
    case kNormal: return want == kFocus || want == kPlot || want == kPalette || want == kBounded || want == kPeriodPalette ||
                         want == kAimed;
    case kPlot: return is_plotted(want) && want != kPlot && want != kAimedBounded;
    case kBounded: return want == kAimedBounded;
    case kFocus:
    case kPalette:
    case kDepth:
    case kDepthPalette:
    case kFrames:
    case kPhoenix:
    case kPeriodPalette:
    case kAimed:
    case kAimedBounded: return false;
  }
  return false;
}

// ---- what the setters and the entry points ask of their own arguments ------------------------------------------------

const double kIdentityProjection[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};

bool projection_ok(const double *p) {
  if (!p) return false;
  for (int j = 0; j < 8; ++j) {
    if (!isfinite(p[j])) return false;
  }
  return true;
}

bool julia_c_ok(const double *c) {  // both in [-2, 2]; a NaN fails the comparisons
  return c && c[0] >= -2.0 && c[0] <= 2.0 && c[1] >= -2.0 && c[1] <= 2.0;
}

bool palette_entries_ok(uint32_t n_entries, const cb_iteration_control *iterations) {
  return n_entries >= 1u && n_entries <= (uint32_t) CB_PALETTE_MAX_ENTRIES && iterations->max_escape_iterations >= 1 &&
         (uint32_t) iterations->max_escape_iterations == n_entries;
}

// A table on the host, in the palette's entry format: the top byte of every entry is zero.
bool lut_host_ok(const uint32_t *lut_host, uint32_t n_entries) {
  if (!lut_host) return false;
  for (uint32_t k = 0; k < n_entries; ++k) {
    if ((lut_host[k] >> 24) != 0u) return false;
  }
  return true;
}

// The depth of a depth render ("Depth render"): finite row and bounds, min < max with a finite difference, N in range, and
// N * h rows still an int (the planes are tone-mapped as one w x N*h image).
bool depth_ok(const cb_depth *d, int h) {
  if (!d) return false;
  for (int j = 0; j < 4; ++j) {
    if (!isfinite(d->row[j])) return false;
  }
  if (!isfinite(d->min) || !isfinite(d->max) || !(d->min < d->max) || !isfinite(d->max - d->min)) return false;
  if (d->slices < 1 || d->slices > CB_DEPTH_MAX_SLICES) return false;
  return (long long) d->slices * (long long) h <= 0x7fffffffLL;
}

// The matrices of a frames render ("Frames render"): F in range, every entry finite, and F * h rows still an int (the
// planes are tone-mapped as one w x F*h image).
bool frames_ok(const double *frames_host, int n_frames, int h) {
  if (!frames_host || n_frames < 1 || n_frames > CB_FRAMES_MAX) return false;
  for (int j = 0; j < 8 * n_frames; ++j) {
    if (!isfinite(frames_host[j])) return false;
  }
  return (long long) n_frames * (long long) h <= 0x7fffffffLL;
}

// The table length and the tolerance of a period-palette render ("Period-palette render"): 2 .. CB_PERIOD_MAX_ENTRIES
// entries, eps finite and >= 0 (a NaN fails the comparisons).
bool period_palette_ok(uint32_t n_entries, double eps) {
  return n_entries >= 2u && n_entries <= (uint32_t) CB_PERIOD_MAX_ENTRIES && eps >= 0.0 && isfinite(eps);
}

// The parameter of a Phoenix render ("Phoenix render"): both parts in [-2, 2]; a NaN fails the comparisons.
bool phoenix_p_ok(const double *p) { return p && p[0] >= -2.0 && p[0] <= 2.0 && p[1] >= -2.0 && p[1] <= 2.0; }

// What every draw entry point asks of its pointers and its canvas.
bool launch_ok(const Launch &l) {
  return l.dims && l.iterations && l.d_hist && l.d_states && l.dims->w > 0 && l.dims->h > 0;
}

// *p = a plotted render of `kind` with this matrix and source of c (julia_c null: c is sampled) and nothing else yet;
// false, *p untouched: a matrix or a c that does not pass.
bool plotted_source(Plotted *p, Kind kind, const double *projection, const double *julia_c) {
  if (!projection_ok(projection) || (julia_c && !julia_c_ok(julia_c))) return false;
  memset(p, 0, sizeof(*p));
  p->kind = kind;
  memcpy(p->projection, projection, sizeof(p->projection));
  if (julia_c) {
    p->julia = true;
    p->julia_c[0] = julia_c[0];
    p->julia_c[1] = julia_c[1];
  }
  return true;
}

// ---- the plotted launch (draw_plot.hip, draw_depth.hip, draw_depth_palette.hip, draw_frames.hip, draw_phoenix.hip,
// draw_bounded.hip, draw_periods.hip) ----

// The arguments all plotted launches share, once the caller's own have passed.  julia_c null: c is sampled; d_lut null: one
// plane, no table.  *lockstep: the variant's base is CB_KERNEL_SIMPLE.  interior false: the launch's step is not the
// Mandelbrot set's, whatever the variant says (draw_phoenix.hip): no map.
int plot_args(const Launch &l, const double projection[8], const double julia_c[2], const uint32_t *d_lut, bool interior,
              cb::PlotArgs *out, bool *lockstep) {
  // A base of two and at most one of: a formula code CB_FORMULA_TRICORN .. CB_FORMULA_MAX ("Formula step"), a degree
  // CB_POWER_MIN .. CB_POWER_MAX ("Multibrot step"), the Burning Ship.  The plotted draws know neither anti nor drain.
  const int kernel_variant = l.kernel_variant;
  const int formula = (kernel_variant & CB_KERNEL_FORMULA_MASK) >> 16;
  const int degree_bits = (kernel_variant & CB_KERNEL_POWER_MASK) >> 12;
  const bool ship = (kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP) != 0;
  const int base_variant = kernel_variant & ~(CB_KERNEL_FORMULA_MASK | CB_KERNEL_POWER_MASK | CB_KERNEL_FLAG_BURNING_SHIP);
  const bool power = degree_bits != 0;
  if ((base_variant != CB_KERNEL_DEFAULT && base_variant != CB_KERNEL_SIMPLE) || formula > CB_FORMULA_MAX ||
      (power && (degree_bits < CB_POWER_MIN || degree_bits > CB_POWER_MAX)) ||
      (formula != 0 ? 1 : 0) + (power ? 1 : 0) + (ship ? 1 : 0) > 1) {
    return (int) hipErrorInvalidValue;
  }
  cb::PlotArgs &pa = *out;
  memset(&pa, 0, sizeof(pa));
  pa.d = make_args(l.dims, l.iterations, l.d_hist, l.d_states, l.n_threads, l.samples_per_thread, l.d_counters, nullptr, 0,
                   nullptr);
  pa.d.burning_ship = ship ? 1 : 0;
  memcpy(pa.p, projection, sizeof(pa.p));
  pa.degree = power ? degree_bits : 2;
  if (julia_c) {
    pa.julia = 1;
    pa.c[0] = julia_c[0];
    pa.c[1] = julia_c[1];
  }
  pa.lut = d_lut;
  pa.plane_pixels = (unsigned long long) l.dims->w * (unsigned long long) l.dims->h;
  pa.formula = formula;
  pa.palette = d_lut ? 1 : 0;
  *lockstep = base_variant == CB_KERNEL_SIMPLE;
  // The interior map (the Mandelbrot set's: a sampled c, degree 2, no formula) where the normal product path consults it:
  // wants_interior_map's rule (not the lock-step kernel, not the Burning Ship, not with the knob), and only when max_iter
  // leaves that path a LONG stage (max_iter > head + mid steps of plan_stages, 20 for min_iter <= 16) -- below that it
  // retires nothing through the map either.
  g_interior_level.store(0, std::memory_order_relaxed);
  if (interior && !julia_c && !power && formula == 0 && pa.d.long_steps > 0) {
    const int rc = attach_interior_map(pa.d, kernel_variant);
    if (rc) return rc;
  }
  return 0;
}

// The step of a plotted launch in its kernel variant: a formula, a degree or the Burning Ship.
constexpr int kStepBits = CB_KERNEL_FORMULA_MASK | CB_KERNEL_POWER_MASK | CB_KERNEL_FLAG_BURNING_SHIP;

// ---- the cell source of the focused and the aimed render (draw_focus.hip, draw_aim.hip) ----

// A probe's level, and a draw's list: level 0 and no cells is the uniform source (the tests' un-listed render through the
// same kernel); else a level in range and a list with entries.
bool cell_level_ok(int level) { return level >= CB_FOCUS_MIN_LEVEL && level <= CB_FOCUS_MAX_LEVEL; }
bool cell_list_ok(int level, const uint32_t *d_cells, uint32_t n_cells) {
  const bool uniform = d_cells == nullptr && n_cells == 0 && level == 0;
  return uniform || (cell_level_ok(level) && d_cells && n_cells > 0);
}

// Probe to list, what cb_renderer_set_focus and cb_renderer_set_aim do once the renderer admits the kind and their own
// arguments have passed: probe_passes passes on generators made afresh from the renderer's seed, in launches of at most
// kRendererPassesPerLaunch -- probe(d_states, samples_per_thread, d_mask) issues one on r->stream --, the mask dilated into
// the list, the list on the device.  0: r->what.cells holds level, list and count (kind and step bits are the caller's).
// Else, `empty` for a mask without a bit included, the renderer is what it was and nothing stays allocated.
template <class Probe>
int probe_cells(cb_renderer *r, int level, uint32_t probe_passes, int dilate, Probe probe, int empty) {
  CB_TRY(hipSetDevice(r->device));
  const size_t mask_bytes = cb_focus_mask_bytes(level);
  void *d_states = nullptr;
  uint32_t *d_mask = nullptr, *d_cells = nullptr;
  std::vector<uint32_t> mask(mask_bytes / sizeof(uint32_t)), cells;
  uint32_t n_cells = 0;
  int rc = (int) hipMalloc(&d_states, cb_rng_state_bytes(r->n_threads));
  if (!rc) rc = (int) hipMalloc(reinterpret_cast<void **>(&d_mask), mask_bytes);
  if (!rc) rc = (int) hipMemsetAsync(d_mask, 0, mask_bytes, r->stream);
  if (!rc) rc = cb_initialize_rng(r->seed, r->first_subsequence, r->n_threads, d_states, r->stream);
  for (uint32_t left = probe_passes; !rc && left > 0;) {
    const uint32_t now = left < kRendererPassesPerLaunch ? left : kRendererPassesPerLaunch;
    rc = probe(d_states, now * CB_SAMPLES_PER_THREAD, d_mask);
    left -= now;
  }
  if (!rc) rc = (int) hipMemcpyAsync(mask.data(), d_mask, mask_bytes, hipMemcpyDeviceToHost, r->stream);
  if (!rc) rc = (int) hipStreamSynchronize(r->stream);
  if (!rc) rc = cb_focus_cells(level, mask.data(), dilate, nullptr, &n_cells);
  if (!rc && n_cells == 0) rc = empty;
  if (!rc) {
    cells.resize(n_cells);
    rc = cb_focus_cells(level, mask.data(), dilate, cells.data(), &n_cells);
  }
  if (!rc) rc = (int) hipMalloc(reinterpret_cast<void **>(&d_cells), (size_t) n_cells * sizeof(uint32_t));
  if (!rc) rc = (int) hipMemcpy(d_cells, cells.data(), (size_t) n_cells * sizeof(uint32_t), hipMemcpyHostToDevice);
  (void) hipFree(d_states);
  (void) hipFree(d_mask);
  if (rc) {
    (void) hipFree(d_cells);
    return rc;
  }
  r->what.cells.level = level;
  r->what.cells.d_cells = d_cells;
  r->what.cells.n_cells = n_cells;
  return 0;
}

// The listed cells and the grid's n * n of a renderer that keeps a list (`listed`), 0 and 0 of one that does not.
int renderer_cells(const cb_renderer *r, bool listed, uint32_t *n_cells, uint32_t *n_total) {
  const uint32_t n = listed ? 4u << r->what.cells.level : 0u;
  if (n_cells) *n_cells = listed ? r->what.cells.n_cells : 0u;
  if (n_total) *n_total = n * n;
  return 0;
}

// One plotted launch: what the ten cb_draw_buddhabrot_{projected .. periods, aimed} entry points and a plotted renderer
// do once their own arguments have passed.  interior_level (may be null): the level of the interior map the launch used, 0 for none
// or when nothing was launched.  cb_debug_last_draw_kernel names the kind and the step, product / lock-step: 8 .. 31
// (cb_aim_probe, which has no histogram, fills its AimArgs itself and reports 30 / 31 as well).
int draw_plotted(const Launch &l, const Plotted &p, int *interior_level) {
  if (interior_level) *interior_level = 0;
  if (!variant_ok(p, l.kernel_variant)) return (int) hipErrorInvalidValue;
  cb::PlotArgs pa;
  bool lockstep = false;
  {
    const int rc = plot_args(l, p.kind == kFrames ? kIdentityProjection : p.projection, p.julia ? p.julia_c : nullptr,
                             p.kind == kPalette ? p.d_lut : nullptr,
                             p.kind != kPhoenix && p.kind != kBounded && p.kind != kPeriodPalette && p.kind != kAimedBounded,
                             &pa, &lockstep);
    if (rc) return rc;
  }
  const hipStream_t stream = reinterpret_cast<hipStream_t>(l.stream);
  const auto report = [lockstep](int id) { g_last_draw_kernel.store(id + (lockstep ? 1 : 0), std::memory_order_relaxed); };
  hipError_t e = hipErrorInvalidValue;
  switch (p.kind) {
    case kNormal:
    case kFocus: break;  // (not plotted: cb_draw_buddhabrot, cb_draw_buddhabrot_focus)
    case kPlot:
    case kPalette:
      report(pa.formula != 0 ? 16 : p.kind == kPalette ? 14 : p.julia ? 12 : pa.degree != 2 ? 10 : 8);
      e = cb::launch_draw_plot(pa, lockstep, stream);
      break;
    case kDepth:
    case kDepthPalette: {  // with a table of n_entries entries on the device: three planes; without: N
      cb::DepthArgs da;
      memset(&da, 0, sizeof(da));
      da.p = pa;
      memcpy(da.row, p.depth.row, sizeof(da.row));
      da.min = p.depth.min;
      da.delta = (p.depth.max - p.depth.min) / (double) p.depth.slices;  // as cb_recompute_pixel_deltas makes delta_imag
      if (!(da.delta > 0.0) || !isfinite(da.delta)) return (int) hipErrorInvalidValue;  // (a window wider than a double)
      da.pow2 = exact_reciprocal(da.delta, &da.inv_delta) ? 1 : 0;
      da.slices = p.depth.slices;
      da.plane_pixels = pa.plane_pixels;
      if (p.kind == kDepthPalette) {
        const cb::DepthPaletteArgs dpa = {da, p.d_lut, da.plane_pixels};
        report(20);
        e = cb::launch_draw_depth_palette(dpa, p.n_entries, lockstep, stream);
      } else {
        report(18);
        e = cb::launch_draw_depth(da, lockstep, stream);
      }
      break;
    }
    case kFrames: {
      cb::FramesArgs fa;
      memset(&fa, 0, sizeof(fa));
      fa.p = pa;
      fa.frames = p.d_frames;
      fa.n_frames = p.n_frames;
      fa.plane_pixels = pa.plane_pixels;
      report(22);
      e = cb::launch_draw_frames(fa, lockstep, stream);
      break;
    }
    case kPhoenix: {  // it knows no interior map
      cb::PhoenixArgs xa;
      memset(&xa, 0, sizeof(xa));
      xa.plot = pa;
      xa.p[0] = p.phoenix_p[0];
      xa.p[1] = p.phoenix_p[1];
      report(24);
      e = cb::launch_draw_phoenix(xa, lockstep, stream);
      break;
    }
    case kBounded:  // nothing is rejected or retired as drawn: no interior map
      report(26);
      e = cb::launch_draw_bounded(pa, lockstep, stream);
      break;
    case kPeriodPalette: {  // the bounded launch with a table keyed by the period: three planes, no interior map
      const cb::PeriodArgs qa = {pa, p.d_lut, (int) p.n_entries, p.period_eps, pa.plane_pixels};
      report(28);
      e = cb::launch_draw_periods(qa, lockstep, stream);
      break;
    }
    case kAimed:
    case kAimedBounded: {  // the projected or the bounded launch from the cell list; the map by plot_args' rule, above
      if ((l.kernel_variant & kStepBits) != p.cells.step_bits) return (int) hipErrorInvalidValue;  // not the probe's step
      cb::AimArgs aa;
      memset(&aa, 0, sizeof(aa));
      aa.p = pa;
      aa.bounded = p.kind == kAimedBounded ? 1 : 0;
      aa.cells = p.cells.d_cells;
      aa.n_cells = p.cells.n_cells;
      cb::set_grid_level(aa, p.cells.level);
      report(30);
      e = cb::launch_draw_aim(aa, lockstep, stream);
      break;
    }
  }
  if (interior_level && e == hipSuccess && pa.d.interior_map) *interior_level = (int) pa.d.interior_shift + 1;
  return (int) e;
}

// Adds one launch (or, with passes == 0, the drain of the carried work) and its flush to the
// renderer's streams.
int enqueue_launch(cb_renderer *r, uint32_t passes, int kernel_variant) {
  if (r->what.kind == kFocus) {  // draw_focus.hip: direct atomics, no deferred scatter, no carry, no interior map
    r->interior_level = 0;
    if (passes == 0) return 0;
    const CellList &c = r->what.cells;
    if ((kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP) != c.step_bits) return (int) hipErrorInvalidValue;
    return cb_draw_buddhabrot_focus(&r->dims, r->d_hist, &r->iterations, r->d_states, r->n_threads,
                                    passes * CB_SAMPLES_PER_THREAD, r->d_counters, kernel_variant, c.level, c.d_cells,
                                    c.n_cells, r->stream);
  }
  if (is_plotted(r->what.kind)) {  // what the setters took is checked
    if (passes == 0) return 0;
    const Launch l = {&r->dims, r->d_hist, &r->iterations, r->d_states, r->n_threads, passes * CB_SAMPLES_PER_THREAD,
                      r->d_counters, kernel_variant, r->stream};
    return draw_plotted(l, r->what, &r->interior_level);
  }
  // the lock-step kernel and the anti kernels: direct atomics, no deferred scatter, no carry
  const bool wave = (kernel_variant & ~kVariantFlags) != CB_KERNEL_SIMPLE && (kernel_variant & CB_KERNEL_FLAG_ANTI) == 0;
  const bool deferred = r->d_workspace[0] && wave;
  const int k = r->next_workspace;
  if (deferred && r->flush_pending[k]) {
    // workspace k is free again once the flush that read it has finished
    CB_TRY(hipStreamWaitEvent(r->stream, r->flush_done[k], 0));
    r->flush_pending[k] = false;
  }
  int rc;
  if (r->n_channels > 0) {
    rc = cb_draw_buddhabrot_channels(&r->dims, r->d_hist, r->windows, r->n_channels, r->d_states,
                                     r->n_threads, passes * CB_SAMPLES_PER_THREAD, r->d_counters,
                                     kernel_variant, deferred ? r->d_workspace[k] : nullptr,
                                     r->workspace_bytes, r->d_carry, r->stream);
  } else {
    rc = cb_draw_buddhabrot(&r->dims, r->d_hist, &r->iterations, r->d_states, r->n_threads,
                            passes * CB_SAMPLES_PER_THREAD, r->d_counters, kernel_variant,
                            deferred ? r->d_workspace[k] : nullptr, r->workspace_bytes,
                            wave ? r->d_carry : nullptr, r->stream);
  }
  if (rc) return rc;
  {
    const DeviceMap *m = wants_interior_map(kernel_variant) ? device_map(kMapInterior) : nullptr;
    r->interior_level = m ? (int) m->level : 0;
  }
  if (wave && r->d_carry) {
    r->carry_pending = passes != 0;
    r->carry_variant = kernel_variant;
  }
  if (deferred) {
    CB_TRY(hipEventRecord(r->draw_done[k], r->stream));
    CB_TRY(hipStreamWaitEvent(r->flush_stream, r->draw_done[k], 0));
    if (r->n_channels > 0) {
      rc = cb_flush_scatter_channels(&r->dims, r->d_hist, r->n_channels, r->n_threads, r->d_workspace[k],
                                     r->workspace_bytes, r->flush_stream);
    } else {
      rc = cb_flush_scatter(&r->dims, r->d_hist, r->n_threads, r->d_workspace[k], r->workspace_bytes,
                            r->flush_stream);
    }
    if (rc) return rc;
    CB_TRY(hipEventRecord(r->flush_done[k], r->flush_stream));
    r->flush_pending[k] = true;
    r->next_workspace = k ^ 1;
  }
  return 0;
}

int sync_streams(cb_renderer *r) {
  CB_TRY(hipStreamSynchronize(r->stream));
  CB_TRY(hipStreamSynchronize(r->flush_stream));
  r->flush_pending[0] = r->flush_pending[1] = false;
  return 0;
}

// Completes the work earlier launches left in the carry buffer: after this the histogram and the
// counters account for every sample drawn so far.
int finish(cb_renderer *r) {
  if (r->carry_pending) {
    int rc = enqueue_launch(r, 0, r->carry_variant);
    if (rc) return rc;
  }
  int rc = sync_streams(r);
  if (rc) return rc;
  // A kernel that saw one of its invariants broken (a queue ring overrun, a replay that does not end) has
  // lost or duplicated samples: the histogram must not be taken for a result.
  unsigned long long status = 0;
  CB_TRY(hipMemcpyAsync(&status, &r->d_counters->status, sizeof(status), hipMemcpyDeviceToHost, r->stream));
  CB_TRY(hipStreamSynchronize(r->stream));
  return status ? CB_ERROR_KERNEL_INVARIANT : 0;
}

// A cleared histogram of `planes` planes in the place of the renderer's first one and, with a table (lut_host not null), a
// device copy of its n_entries in *d_lut: what the setters of a palette, a depth and a depth palette do once the renderer
// has passed as theirs.  On failure nothing is kept and the renderer is as it was.
int swap_in_planes(cb_renderer *r, size_t planes, const uint32_t *lut_host, uint32_t n_entries, const uint32_t **d_lut) {
  CB_TRY(hipSetDevice(r->device));
  CB_TRY(hipStreamSynchronize(r->stream));  // (the histogram's first memset)
  const size_t hist_bytes = planes * (size_t) r->dims.w * (size_t) r->dims.h * sizeof(cb_pixel);
  const size_t lut_bytes = (size_t) n_entries * sizeof(uint32_t);
  cb_pixel *d_hist = nullptr;
  uint32_t *d_table = nullptr;
  int rc = (int) hipMalloc(reinterpret_cast<void **>(&d_hist), hist_bytes);
  if (!rc && lut_host) rc = (int) hipMalloc(reinterpret_cast<void **>(&d_table), lut_bytes);
  if (!rc) rc = (int) hipMemsetAsync(d_hist, 0, hist_bytes, r->stream);
  if (!rc && lut_host) rc = (int) hipMemcpyAsync(d_table, lut_host, lut_bytes, hipMemcpyHostToDevice, r->stream);
  if (!rc) rc = (int) hipStreamSynchronize(r->stream);  // lut_host is the caller's
  if (rc) {
    (void) hipFree(d_hist);
    (void) hipFree(d_table);
    return rc;
  }
  (void) hipFree(r->d_hist);
  r->d_hist = d_hist;
  if (lut_host) *d_lut = d_table;
  return 0;
}

// The tone map of `rows` rows of w counters at `hist`, exposed as the renderer is set: plainly, against the white point of
// its clip, equalised, or locally equalised: the rows are then planes of `plane_h` rows that share the tiles' tables.  The
// renderer keeps what the call found.
int tone_map_counters(cb_renderer *r, const cb_pixel *hist, int rows, int plane_h, double gamma, int mode,
                      uint16_t *d_gray_be, uint64_t *max_out, double *scale_out) {
  cb::Exposure how = {r->equalize ? cb::Exposure::kEqualized
                                  : (r->white_clip != 0.0 ? cb::Exposure::kWhiteClip : cb::Exposure::kPlain),
                      r->white_clip};
  if (r->local_tiles_x != 0) {
    if (plane_h <= 0 || rows % plane_h != 0) return (int) hipErrorInvalidValue;
    how.kind = cb::Exposure::kLocalEqualized;
    how.planes = rows / plane_h;
    how.tiles_x = r->local_tiles_x;
    how.tiles_y = r->local_tiles_y;
    how.clip_q = r->local_clip_q;
  }
  const int rc = cb::tone_map_exposed(reinterpret_cast<const unsigned long long *>(hist), r->dims.w, rows, gamma, mode, how,
                                      d_gray_be, &r->last_exposed, r->stream);
  if (rc) return rc;
  const cb::Exposed &e = r->last_exposed;
  if (max_out) *max_out = e.max;  // the true maximum, and the scale applied
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) (how.kind == cb::Exposure::kWhiteClip ? e.white : e.max));
  return 0;
}

// The one tone-map call of every image: `rows` rows of w counters at `hist`, planes of `plane_h` rows each that are
// smoothed in groups of `group` where the renderer has a density filter.  The filtered counters live for this call only.
int tone_map_rows(cb_renderer *r, const cb_pixel *hist, int rows, int plane_h, int group, double gamma, int mode,
                  uint16_t *d_gray_be, uint64_t *max_out, double *scale_out) {
  if (r->density_radius == 0) return tone_map_counters(r, hist, rows, plane_h, gamma, mode, d_gray_be, max_out, scale_out);
  if (plane_h <= 0 || rows % plane_h != 0) return (int) hipErrorInvalidValue;
  cb_pixel *d_filtered = nullptr;
  CB_TRY(hipMalloc(reinterpret_cast<void **>(&d_filtered), (size_t) rows * (size_t) r->dims.w * sizeof(cb_pixel)));
  int rc = cb_density_filter_device(hist, r->dims.w, plane_h, rows / plane_h, group, r->density_radius,
                                    r->density_thresholds, d_filtered, r->stream);
  if (rc == 0) rc = tone_map_counters(r, d_filtered, rows, plane_h, gamma, mode, d_gray_be, max_out, scale_out);  // synchronises
  (void) hipFree(d_filtered);
  return rc;
}

// `rows` rows of the histogram from `plane` on as one w x rows image, one maximum for all of it: finish, tone-map, copy
// out.  What cb_renderer_grayscale_plane (one plane) and kind_image (all of them) do after their checks.
int gray_image(cb_renderer *r, size_t plane, int rows, double gamma, int mode, uint16_t *host_gray_be, uint64_t *max_out,
               double *scale_out) {
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  const size_t bytes = (size_t) rows * (size_t) r->dims.w * sizeof(uint16_t);
  uint16_t *d_gray = nullptr;
  CB_TRY(hipMalloc(reinterpret_cast<void **>(&d_gray), bytes));
  int rc = tone_map_rows(r, r->d_hist + plane * (size_t) r->dims.w * (size_t) r->dims.h, rows, r->dims.h, 1, gamma, mode,
                         d_gray, max_out, scale_out);
  if (rc == 0) rc = (int) hipMemcpyAsync(host_gray_be, d_gray, bytes, hipMemcpyDeviceToHost, r->stream);
  if (rc == 0) rc = (int) hipStreamSynchronize(r->stream);
  (void) hipFree(d_gray);
  return rc;
}

__global__ void __launch_bounds__(256) add_histogram_kernel(unsigned long long *dst,
                                                            const unsigned long long *src, size_t n) {
  const size_t stride = (size_t) gridDim.x * blockDim.x;
  for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] += src[i];
}

// ncclReduce of the renderers' histograms onto renderers[0] (one device each).  librccl is opened on
// first use; the symbols are the ones rccl.h declares.
std::mutex g_rccl_mutex;
decltype(&ncclCommDestroy) g_comm_destroy = nullptr;
std::vector<int> g_comm_devices;   // the devices of the cached communicators ...
std::vector<ncclComm_t> g_comms;   // ... one per device, kept until one of their renderers goes (below)

// The cached communicators end with the first renderer of their set that is destroyed (cb_renderer_destroy): nothing of
// RCCL's is left to the teardown of the process.
void release_communicators_with(int device) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  bool mine = false;
  for (int d : g_comm_devices) mine = mine || d == device;
  if (!mine || !g_comm_destroy) return;
  for (ncclComm_t c : g_comms) (void) g_comm_destroy(c);
  g_comms.clear();
  g_comm_devices.clear();
}

int rccl_reduce_to_root(cb_renderer *const *renderers, int n, size_t count) {
  static void *lib = nullptr;
  static decltype(&ncclCommInitAll) comm_init_all = nullptr;
  static decltype(&ncclGroupStart) group_start = nullptr;
  static decltype(&ncclGroupEnd) group_end = nullptr;
  static decltype(&ncclReduce) reduce = nullptr;
  decltype(&ncclCommDestroy) &comm_destroy = g_comm_destroy;
  std::vector<int> &comm_devices = g_comm_devices;
  std::vector<ncclComm_t> &comms = g_comms;
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (!lib) {
    lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return (int) hipErrorSharedObjectInitFailed;
    comm_init_all = reinterpret_cast<decltype(comm_init_all)>(dlsym(lib, "ncclCommInitAll"));
    comm_destroy = reinterpret_cast<decltype(&ncclCommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    group_start = reinterpret_cast<decltype(group_start)>(dlsym(lib, "ncclGroupStart"));
    group_end = reinterpret_cast<decltype(group_end)>(dlsym(lib, "ncclGroupEnd"));
    reduce = reinterpret_cast<decltype(reduce)>(dlsym(lib, "ncclReduce"));
    if (!comm_init_all || !comm_destroy || !group_start || !group_end || !reduce) {
      return (int) hipErrorSharedObjectSymbolNotFound;
    }
  }
  std::vector<int> devices(n);
  for (int k = 0; k < n; ++k) devices[k] = renderers[k]->device;
  // One communicator per set of devices, kept while its renderers live: creating it costs far more than the reduce (a
  // bootstrap over all ranks), and a renderer set is reduced at every checkpoint.
  if (comm_devices != devices) {
    for (ncclComm_t c : comms) (void) comm_destroy(c);
    comms.assign((size_t) n, nullptr);
    comm_devices.clear();
    if (comm_init_all(comms.data(), n, devices.data()) != ncclSuccess) {
      comms.clear();
      return (int) hipErrorUnknown;
    }
    comm_devices = devices;
  }
  ncclResult_t nr = group_start();
  for (int k = 0; k < n && nr == ncclSuccess; ++k) {
    if (hipSetDevice(devices[k]) != hipSuccess) {
      nr = ncclUnhandledCudaError;
      break;
    }
    // in place on the root; u64 counters, integer sum: the result does not depend on the order
    nr = reduce(renderers[k]->d_hist, renderers[k]->d_hist, count, ncclUint64, ncclSum, 0, comms[k],
                renderers[k]->stream);
  }
  const ncclResult_t ne = group_end();
  int rc = (nr == ncclSuccess && ne == ncclSuccess) ? 0 : (int) hipErrorUnknown;
  for (int k = 0; k < n; ++k) {
    (void) hipSetDevice(devices[k]);
    const hipError_t e = hipStreamSynchronize(renderers[k]->stream);
    if (e != hipSuccess && rc == 0) rc = (int) e;
  }
  if (rc != 0) {  // a communicator that has failed is not reused
    for (ncclComm_t c : comms) (void) comm_destroy(c);
    comms.clear();
    comm_devices.clear();
  }
  return rc;
}

}  // namespace

extern "C" {

int cb_abi_version(void) { return CB_ABI_VERSION; }

int cb_debug_last_draw_kernel(void) { return g_last_draw_kernel.load(std::memory_order_relaxed); }
int cb_debug_interior_map_level(void) { return g_interior_level.load(std::memory_order_relaxed); }
int cb_renderer_interior_map_level(const cb_renderer *r) { return r ? r->interior_level : 0; }

const char *cb_error_string(int code) {
  if (code == 0) return "no error";
  if (code == CB_ERROR_KERNEL_INVARIANT) {
    return "the draw kernel reported a broken internal invariant (cb_counters.status): samples were lost";
  }
  if (code == CB_ERROR_FOCUS_EMPTY) {
    return "the focus probe marked no cell: no probed sample has an accepted orbit that enters the canvas";
  }
  if (code == CB_ERROR_AIM_EMPTY) {
    return "the aim probe marked no cell: no probed sample has a plotted orbit that enters the canvas";
  }
  return hipGetErrorString((hipError_t) code);
}

int cb_initialize_rng(uint64_t seed, uint64_t first_subsequence, uint32_t n_threads, void *d_states,
                      void *stream) {
  if (n_threads == 0) return 0;
  if (!d_states) return (int) hipErrorInvalidValue;
  const uint32_t *mats = nullptr;
  int rc = device_matrices(&mats);
  if (rc) return rc;
  return (int) cb::launch_rng_init(seed, first_subsequence, n_threads,
                                   reinterpret_cast<uint32_t *>(d_states), mats,
                                   reinterpret_cast<hipStream_t>(stream));
}

size_t cb_carry_bytes(uint32_t n_threads) {
  return (size_t) cb::draw_wave_count(n_threads) * cb::kCarryWordsPerWave * sizeof(unsigned long long) +
         (size_t) cb::kSchedWords * sizeof(uint32_t);
}

size_t cb_scatter_workspace_bytes_channels(const cb_fractal_dimensions *dims, int n_channels, uint32_t n_threads,
                                           uint32_t samples_per_thread) {
  if (!dims || dims->w <= 0 || dims->h <= 0 || n_threads == 0 || samples_per_thread == 0) return 0;
  if (n_channels < 1 || n_channels > CB_MAX_CHANNELS) return 0;
  const uint32_t n_waves = cb::draw_wave_count(n_threads);
  // every plane of a fused launch receives its own share of the visited points
  const double entries = (double) n_threads * (double) samples_per_thread * kEntriesPerSample * (n_channels > 1 ? 1.5 : 1.0);
  return cb::bin_workspace_bytes(dims->w, dims->h, n_waves, entries / n_waves, n_channels);
}

size_t cb_scatter_workspace_bytes(const cb_fractal_dimensions *dims, uint32_t n_threads,
                                  uint32_t samples_per_thread) {
  return cb_scatter_workspace_bytes_channels(dims, 1, n_threads, samples_per_thread);
}

int cb_draw_buddhabrot(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                       const cb_iteration_control *iterations, void *d_states, uint32_t n_threads,
                       uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                       void *d_workspace, size_t workspace_bytes, void *d_carry, void *stream) {
  if (!dims || !iterations || !d_hist || !d_states) return (int) hipErrorInvalidValue;
  if (dims->w <= 0 || dims->h <= 0) return (int) hipErrorInvalidValue;
  if ((kernel_variant & (CB_KERNEL_POWER_MASK | CB_KERNEL_FORMULA_MASK)) != 0) {
    return (int) hipErrorInvalidValue;  // a degree, a formula: projected renders only
  }
  const bool ship = (kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP) != 0;
  const int base_variant = kernel_variant & ~kVariantFlags;
  const bool anti = (kernel_variant & CB_KERNEL_FLAG_ANTI) != 0;
  if (anti && base_variant != CB_KERNEL_DEFAULT && base_variant != CB_KERNEL_SIMPLE) return (int) hipErrorInvalidValue;
  if (base_variant == CB_KERNEL_SIMPLE || anti) {  // the baseline and the anti kernels: atomics, every launch complete
    d_workspace = nullptr;
    d_carry = nullptr;
  }
  cb::DrawArgs a = make_args(dims, iterations, d_hist, d_states, n_threads, samples_per_thread,
                             d_counters, d_workspace, workspace_bytes, d_carry);
  a.burning_ship = ship ? 1 : 0;
  a.anti = anti ? 1 : 0;
  if ((kernel_variant & CB_KERNEL_FLAG_DRAIN) && a.carry) a.drain = 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  {
    int rc = empty_stream_if_nothing_launches(a, s);
    if (rc) return rc;
  }
  const auto wave = ship ? cb::launch_draw_wave_ship : cb::launch_draw_wave;
  {
    const int rc = attach_interior_map(a, kernel_variant);
    if (rc) return rc;
  }
  if (anti) {  // draw_anti.hip: the product kernel (4) or the lock-step one (5)
    const bool lockstep = base_variant == CB_KERNEL_SIMPLE;
    g_last_draw_kernel.store(lockstep ? 5 : 4, std::memory_order_relaxed);
    return (int) cb::launch_draw_anti(a, lockstep, s);
  }
  // the two-waves-per-SIMD kernel where it applies (CUDABROT_AMD_NO_WIDE=1, a test knob: never)
  const bool wide = cb::draw_wide_takes(a) && cb_debug_knob("CUDABROT_AMD_NO_WIDE") == nullptr;
  const auto wide_launch = ship ? cb::launch_draw_wide_ship : cb::launch_draw_wide;
  g_last_draw_kernel.store(base_variant == CB_KERNEL_SIMPLE ? 3 : (wide ? 2 : 1), std::memory_order_relaxed);
  switch (base_variant) {
    case CB_KERNEL_DEFAULT:
      return (int) (wide ? wide_launch(a, false, s) : wave(a, false, s));
    case CB_KERNEL_FULL_ITERATE:
      a.check_periodic = 0;
      return (int) (wide ? wide_launch(a, false, s) : wave(a, false, s));
    case CB_KERNEL_TIMED:
      if (cb_debug_knob("CUDABROT_AMD_TIMED_FULL")) a.check_periodic = 0;  // diagnostic: stage clocks of the full-iterate form
      return (int) (wide ? wide_launch(a, true, s) : wave(a, true, s));
    case CB_KERNEL_SIMPLE:
      return (int) cb::launch_draw_simple(a, s);
    default:
      return (int) hipErrorInvalidValue;
  }
}

int cb_flush_scatter(const cb_fractal_dimensions *dims, cb_pixel *d_hist, uint32_t n_threads,
                     void *d_workspace, size_t workspace_bytes, void *stream) {
  if (!dims || !d_hist || dims->w <= 0 || dims->h <= 0) return (int) hipErrorInvalidValue;
  // the carve is a pure function of these arguments, so it is the one the draw call used
  const cb::BinLayout b = cb::make_bin_layout(d_workspace, workspace_bytes, dims->w, dims->h,
                                              cb::draw_wave_count(n_threads));
  return (int) cb::launch_binned_scatter(b, reinterpret_cast<unsigned long long *>(d_hist), dims->w,
                                         dims->h, reinterpret_cast<hipStream_t>(stream));
}

int cb_draw_buddhabrot_channels(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                const cb_iteration_control *windows, int n_channels, void *d_states,
                                uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                int kernel_variant, void *d_workspace, size_t workspace_bytes,
                                void *d_carry, void *stream) {
  if (!dims || !windows || !d_hist || !d_states) return (int) hipErrorInvalidValue;
  if (dims->w <= 0 || dims->h <= 0 || n_channels < 1 || n_channels > CB_MAX_CHANNELS) {
    return (int) hipErrorInvalidValue;
  }
  const bool ship = (kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP) != 0;
  const int base_variant = kernel_variant & ~kVariantFlags;  // a Multibrot degree or a formula stays in it and is refused below
  if ((base_variant != CB_KERNEL_DEFAULT && base_variant != CB_KERNEL_FULL_ITERATE) ||
      (kernel_variant & CB_KERNEL_FLAG_ANTI) != 0) {
    return (int) hipErrorInvalidValue;  // the wave-scheduled kernel only; no anti channels
  }
  // the kernel iterates to the largest max; what escapes before the smallest min is in no window
  cb_iteration_control hull = windows[0];
  for (int j = 1; j < n_channels; ++j) {
    if (windows[j].max_escape_iterations > hull.max_escape_iterations) {
      hull.max_escape_iterations = windows[j].max_escape_iterations;
    }
    if (windows[j].min_escape_iterations < hull.min_escape_iterations) {
      hull.min_escape_iterations = windows[j].min_escape_iterations;
    }
  }
  cb::DrawArgs a = make_args(dims, &hull, d_hist, d_states, n_threads, samples_per_thread, d_counters,
                             d_workspace, workspace_bytes, d_carry, n_channels);
  a.burning_ship = ship ? 1 : 0;
  if ((kernel_variant & CB_KERNEL_FLAG_DRAIN) && a.carry) a.drain = 1;
  a.n_channels = n_channels;
  a.plane_pixels = (unsigned long long) dims->w * (unsigned long long) dims->h;
  for (int j = 0; j < n_channels; ++j) {
    a.chan_min[j] = windows[j].min_escape_iterations;
    a.chan_max[j] = windows[j].max_escape_iterations;
  }
  if (base_variant == CB_KERNEL_FULL_ITERATE) a.check_periodic = 0;
  {
    int rc = empty_stream_if_nothing_launches(a, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc;
  }
  {
    const int rc = attach_interior_map(a, kernel_variant);
    if (rc) return rc;
  }
  const auto wave = ship ? cb::launch_draw_wave_ship : cb::launch_draw_wave;
  g_last_draw_kernel.store(1, std::memory_order_relaxed);
  return (int) wave(a, false, reinterpret_cast<hipStream_t>(stream));
}

int cb_flush_scatter_channels(const cb_fractal_dimensions *dims, cb_pixel *d_hist, int n_channels,
                              uint32_t n_threads, void *d_workspace, size_t workspace_bytes,
                              void *stream) {
  if (!dims || !d_hist || dims->w <= 0 || dims->h <= 0 || n_channels < 1 || n_channels > CB_MAX_CHANNELS) {
    return (int) hipErrorInvalidValue;
  }
  // every word carries the index of its plane and the planes are sorted as one canvas: one pass
  const cb::BinLayout b = cb::make_bin_layout(d_workspace, workspace_bytes, dims->w, dims->h,
                                              cb::draw_wave_count(n_threads), n_channels);
  return (int) cb::launch_binned_scatter(b, reinterpret_cast<unsigned long long *>(d_hist), dims->w, dims->h,
                                         reinterpret_cast<hipStream_t>(stream));
}

int cb_debug_scatter_layout(const cb_fractal_dimensions *dims, int n_channels, uint32_t n_threads,
                            const void *d_workspace, size_t workspace_bytes, cb_scatter_layout *out) {
  if (!dims || !out || dims->w <= 0 || dims->h <= 0 || n_channels < 0 || n_channels > CB_MAX_CHANNELS) {
    return (int) hipErrorInvalidValue;
  }
  // the carve of the draw and flush entry points above, and nothing else: the workspace is not touched
  cb::BinLayoutBytes carved;
  const cb::BinLayout b = cb::make_bin_layout(const_cast<void *>(d_workspace), workspace_bytes, dims->w, dims->h,
                                              cb::draw_wave_count(n_threads), n_channels, &carved);
  memset(out, 0, sizeof(*out));
  out->enabled = b.enabled;
  out->n_waves = b.n_waves;
  out->n_planes = b.n_planes;
  out->e_row_shift = b.e_row_shift;
  out->e_col_mask = b.e_col_mask;
  out->e_row_mask = b.e_row_mask;
  out->e_chan_shift = b.e_chan_shift;
  out->e_chan_mask = b.e_chan_mask;
  if (!b.enabled) return 0;
  out->cap = b.cap;
  out->n_tiles = b.n_tiles;
  out->tiles_x = b.tiles_x;
  out->tiles_y = b.tiles_y;
  out->two_level = b.two_level;
  out->n_groups = b.n_groups;
  out->chunked = b.chunked;
  out->chunks_per_wave = b.chunks_per_wave;
  out->max_regions = b.max_regions;
  const auto place = [&](const void *p, size_t bytes) {
    cb_scatter_array a = {0, 0};
    if (p) {
      a.offset = (uint64_t) (reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(d_workspace));
      a.bytes = (uint64_t) bytes;
    }
    return a;
  };
#define CB_PLACE(name) out->name = place(b.name, carved.name)
  CB_PLACE(wave_count);
  CB_PLACE(stream);
  CB_PLACE(a_count);
  CB_PLACE(a_base);
  CB_PLACE(grouped);
  CB_PLACE(region_start);
  CB_PLACE(region_count);
  CB_PLACE(region_group);
  CB_PLACE(owner_first);
  CB_PLACE(group_first);
  CB_PLACE(group_regions);
  CB_PLACE(n_regions);
  CB_PLACE(chunk_desc);
  CB_PLACE(chunk_list);
  CB_PLACE(run_start);
  CB_PLACE(slice_base);
  CB_PLACE(sorted);
#undef CB_PLACE
  return 0;
}

// ---- focused render (draw_focus.hip; include/cudabrot_amd.h, "Focused render") --------------------------------------

namespace {

// CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, optionally with the Burning Ship's flag: everything a focus launch accepts (a
// Multibrot degree, CB_KERNEL_POWER_MASK, or a formula, CB_KERNEL_FORMULA_MASK, is one of the other bits).
bool focus_variant_ok(int kernel_variant) {
  const int base_variant = kernel_variant & ~CB_KERNEL_FLAG_BURNING_SHIP;
  return base_variant == CB_KERNEL_DEFAULT || base_variant == CB_KERNEL_SIMPLE;
}

int launch_focus(cb::FocusArgs &f, int level, int kernel_variant, hipStream_t stream) {
  f.d.burning_ship = (kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP) != 0 ? 1 : 0;
  cb::set_grid_level(f.g, level);
  const bool lockstep = (kernel_variant & ~CB_KERNEL_FLAG_BURNING_SHIP) == CB_KERNEL_SIMPLE;
  g_last_draw_kernel.store(lockstep ? 7 : 6, std::memory_order_relaxed);
  g_interior_level.store(0, std::memory_order_relaxed);
  return (int) cb::launch_draw_focus(f, lockstep, stream);
}

}  // namespace

int cb_focus_probe(const cb_fractal_dimensions *dims, const cb_iteration_control *iterations, void *d_states,
                   uint32_t n_threads, uint32_t samples_per_thread, int level, uint32_t *d_mask,
                   cb_counters *d_counters, int kernel_variant, void *stream) {
  if (!dims || !iterations || !d_states || !d_mask || dims->w <= 0 || dims->h <= 0) return (int) hipErrorInvalidValue;
  if (!cell_level_ok(level) || !focus_variant_ok(kernel_variant)) return (int) hipErrorInvalidValue;
  cb::FocusArgs f;
  memset(&f, 0, sizeof(f));
  f.d = make_args(dims, iterations, nullptr, d_states, n_threads, samples_per_thread, d_counters, nullptr, 0, nullptr);
  f.g.mask = d_mask;
  return launch_focus(f, level, kernel_variant, reinterpret_cast<hipStream_t>(stream));
}

int cb_draw_buddhabrot_focus(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                             const cb_iteration_control *iterations, void *d_states, uint32_t n_threads,
                             uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, int level,
                             const uint32_t *d_cells, uint32_t n_cells, void *stream) {
  if (!dims || !iterations || !d_hist || !d_states || dims->w <= 0 || dims->h <= 0) return (int) hipErrorInvalidValue;
  if (!focus_variant_ok(kernel_variant) || !cell_list_ok(level, d_cells, n_cells)) return (int) hipErrorInvalidValue;
  cb::FocusArgs f;
  memset(&f, 0, sizeof(f));
  f.d = make_args(dims, iterations, d_hist, d_states, n_threads, samples_per_thread, d_counters, nullptr, 0, nullptr);
  f.g.cells = d_cells;
  f.g.n_cells = n_cells;
  return launch_focus(f, level, kernel_variant, reinterpret_cast<hipStream_t>(stream));
}

int cb_renderer_set_focus(cb_renderer *r, int level, uint32_t probe_passes, int dilate, int kernel_variant) {
  if (!admits(r, kFocus) || probe_passes == 0 || dilate < 0 || !cell_level_ok(level) || !focus_variant_ok(kernel_variant)) {
    return (int) hipErrorInvalidValue;
  }
  const auto probe = [=](void *d_states, uint32_t samples_per_thread, uint32_t *d_mask) {
    return cb_focus_probe(&r->dims, &r->iterations, d_states, r->n_threads, samples_per_thread, level, d_mask, nullptr,
                          kernel_variant, r->stream);
  };
  const int rc = probe_cells(r, level, probe_passes, dilate, probe, CB_ERROR_FOCUS_EMPTY);
  if (rc) return rc;
  r->what.kind = kFocus;
  r->what.cells.step_bits = kernel_variant & CB_KERNEL_FLAG_BURNING_SHIP;
  return 0;
}

int cb_renderer_focus_cells(const cb_renderer *r, uint32_t *n_cells, uint32_t *n_total) {
  if (!r) return (int) hipErrorInvalidValue;
  return renderer_cells(r, r->what.kind == kFocus, n_cells, n_total);
}

// ---- the plotted renders (include/cudabrot_amd.h, "Projected render" .. "Phoenix render") ----------------------------
//
// Every entry point: the shared checks, its own, fill, draw_plotted.  Every setter: `admits`, its own checks, then the
// renderer becomes what was asked for.

int cb_draw_buddhabrot_projected(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                 const cb_iteration_control *iterations, const double projection[8], void *d_states,
                                 uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                 int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kPlot, projection, nullptr)) return (int) hipErrorInvalidValue;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_projection(cb_renderer *r, const double projection[8]) {
  if (!admits(r, kPlot) || !plotted_source(&r->what, kPlot, projection, nullptr)) return (int) hipErrorInvalidValue;
  return 0;
}

int cb_renderer_projection(const cb_renderer *r, double out[8]) {
  if (!r || !out || !is_plotted(r->what.kind)) return 0;
  memcpy(out, r->what.projection, sizeof(r->what.projection));
  return 1;
}

int cb_draw_buddhabrot_julia(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2], void *d_states, uint32_t n_threads,
                             uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !julia_c || !plotted_source(&p, kPlot, projection, julia_c)) return (int) hipErrorInvalidValue;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_julia(cb_renderer *r, const double projection[8], const double julia_c[2]) {
  if (!admits(r, kPlot) || !julia_c ||
      !plotted_source(&r->what, kPlot, projection ? projection : kIdentityProjection, julia_c)) {
    return (int) hipErrorInvalidValue;
  }
  return 0;
}

int cb_renderer_julia(const cb_renderer *r, double out[2]) {
  if (!r || !out || !r->what.julia) return 0;
  out[0] = r->what.julia_c[0];
  out[1] = r->what.julia_c[1];
  return 1;
}

namespace {

// out[3 i + j] = planes[j n + i]: the three planes of big-endian values as the R, G, B of a PPM body.
__global__ void __launch_bounds__(256) interleave_planes_kernel(const uint16_t *planes, size_t n, uint16_t *out) {
  const size_t stride = (size_t) gridDim.x * blockDim.x;
  for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    out[3 * i + 0] = planes[i];
    out[3 * i + 1] = planes[n + i];
    out[3 * i + 2] = planes[2 * n + i];
  }
}

}  // namespace

int cb_draw_buddhabrot_palette(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2], const uint32_t *d_lut,
                               uint32_t n_entries, void *d_states, uint32_t n_threads, uint32_t samples_per_thread,
                               cb_counters *d_counters, int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kPalette, projection, julia_c)) return (int) hipErrorInvalidValue;
  if (!d_lut || !palette_entries_ok(n_entries, iterations)) return (int) hipErrorInvalidValue;
  p.d_lut = d_lut;
  p.n_entries = n_entries;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_palette(cb_renderer *r, const uint32_t *lut_host, uint32_t n_entries) {
  if (!admits(r, kPalette) || !palette_entries_ok(n_entries, &r->iterations) || !lut_host_ok(lut_host, n_entries)) {
    return (int) hipErrorInvalidValue;
  }
  const int rc = swap_in_planes(r, 3, lut_host, n_entries, &r->what.d_lut);
  if (rc) return rc;
  if (r->what.kind == kNormal) memcpy(r->what.projection, kIdentityProjection, sizeof(r->what.projection));  // alone
  r->what.n_entries = n_entries;
  r->what.kind = kPalette;
  return 0;
}

int cb_renderer_palette(const cb_renderer *r, uint32_t *n_entries) {
  if (!r || r->what.kind != kPalette) return 0;
  if (n_entries) *n_entries = r->what.n_entries;
  return 1;
}

int cb_draw_buddhabrot_depth(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2], const cb_depth *depth, void *d_states,
                             uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                             void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kDepth, projection, julia_c)) return (int) hipErrorInvalidValue;
  if (!depth_ok(depth, dims->h)) return (int) hipErrorInvalidValue;
  p.depth = *depth;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_depth(cb_renderer *r, const cb_depth *depth) {
  if (!admits(r, kDepth) || !depth_ok(depth, r->dims.h)) return (int) hipErrorInvalidValue;
  const int rc = swap_in_planes(r, (size_t) depth->slices, nullptr, 0u, nullptr);
  if (rc) return rc;
  r->what.depth = *depth;
  r->what.kind = kDepth;
  return 0;
}

int cb_renderer_depth(const cb_renderer *r, cb_depth *out) {
  if (!r || r->what.kind != kDepth) return 0;
  if (out) *out = r->what.depth;
  return r->what.depth.slices;
}

int cb_draw_buddhabrot_depth_palette(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                     const cb_iteration_control *iterations, const double projection[8],
                                     const double julia_c[2], const cb_depth *depth, const uint32_t *d_lut, uint32_t n_entries,
                                     void *d_states, uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                     int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kDepthPalette, projection, julia_c)) return (int) hipErrorInvalidValue;
  if (!depth_ok(depth, dims->h) || !d_lut || n_entries != (uint32_t) depth->slices) return (int) hipErrorInvalidValue;
  p.depth = *depth;
  p.d_lut = d_lut;
  p.n_entries = n_entries;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_depth_palette(cb_renderer *r, const cb_depth *depth, const uint32_t *lut_host, uint32_t n_entries) {
  if (!admits(r, kDepthPalette) || !depth_ok(depth, r->dims.h) || n_entries != (uint32_t) depth->slices ||
      !lut_host_ok(lut_host, n_entries)) {
    return (int) hipErrorInvalidValue;
  }
  const int rc = swap_in_planes(r, 3, lut_host, n_entries, &r->what.d_lut);
  if (rc) return rc;
  r->what.depth = *depth;
  r->what.n_entries = n_entries;
  r->what.kind = kDepthPalette;
  return 0;
}

int cb_renderer_depth_palette(const cb_renderer *r, cb_depth *out, uint32_t *n_entries) {
  if (!r || r->what.kind != kDepthPalette) return 0;
  if (out) *out = r->what.depth;
  if (n_entries) *n_entries = r->what.n_entries;
  return 1;
}

int cb_draw_buddhabrot_frames(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                              const double *d_frames, int n_frames, const double julia_c[2], void *d_states,
                              uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                              void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kFrames, kIdentityProjection, julia_c)) return (int) hipErrorInvalidValue;
  if (!d_frames || n_frames < 1 || n_frames > CB_FRAMES_MAX) return (int) hipErrorInvalidValue;
  // the matrices are the caller's device memory: their entries are looked at in a host copy, made on the caller's stream
  std::vector<double> copy(8 * (size_t) n_frames);
  CB_TRY(hipMemcpyAsync(copy.data(), d_frames, copy.size() * sizeof(double), hipMemcpyDeviceToHost,
                        reinterpret_cast<hipStream_t>(stream)));
  CB_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  if (!frames_ok(copy.data(), n_frames, dims->h)) return (int) hipErrorInvalidValue;
  p.d_frames = d_frames;
  p.n_frames = n_frames;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_frames(cb_renderer *r, const double *frames_host, int n_frames) {
  if (!admits(r, kFrames) || !frames_ok(frames_host, n_frames, r->dims.h)) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  const size_t bytes = 8 * (size_t) n_frames * sizeof(double);
  double *d_frames = nullptr;
  CB_TRY(hipMalloc(reinterpret_cast<void **>(&d_frames), bytes));
  int rc = (int) hipMemcpy(d_frames, frames_host, bytes, hipMemcpyHostToDevice);
  if (!rc) rc = swap_in_planes(r, (size_t) n_frames, nullptr, 0u, nullptr);
  if (rc) {
    (void) hipFree(d_frames);
    return rc;
  }
  r->frames = new std::vector<double>(frames_host, frames_host + 8 * (size_t) n_frames);
  r->what.d_frames = d_frames;
  r->what.n_frames = n_frames;
  r->what.kind = kFrames;
  return 0;
}

int cb_renderer_frames(const cb_renderer *r, double *out) {
  if (!r || r->what.kind != kFrames) return 0;
  if (out) memcpy(out, r->frames->data(), r->frames->size() * sizeof(double));
  return r->what.n_frames;
}

int cb_draw_buddhabrot_phoenix(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2], const double phoenix_p[2],
                               void *d_states, uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                               int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kPhoenix, projection, julia_c)) return (int) hipErrorInvalidValue;
  if (!phoenix_p_ok(phoenix_p)) return (int) hipErrorInvalidValue;
  p.phoenix_p[0] = phoenix_p[0];
  p.phoenix_p[1] = phoenix_p[1];
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_phoenix(cb_renderer *r, const double phoenix_p[2]) {
  if (!admits(r, kPhoenix) || !phoenix_p_ok(phoenix_p)) return (int) hipErrorInvalidValue;  // the histogram stays one plane
  r->what.phoenix_p[0] = phoenix_p[0];
  r->what.phoenix_p[1] = phoenix_p[1];
  r->what.kind = kPhoenix;
  return 0;
}

int cb_renderer_phoenix(const cb_renderer *r, double out[2]) {
  if (!r || !out || r->what.kind != kPhoenix) return 0;
  out[0] = r->what.phoenix_p[0];
  out[1] = r->what.phoenix_p[1];
  return 1;
}

int cb_draw_buddhabrot_bounded(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2], void *d_states, uint32_t n_threads,
                               uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kBounded, projection, julia_c)) return (int) hipErrorInvalidValue;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_bounded(cb_renderer *r) {
  if (!admits(r, kBounded)) return (int) hipErrorInvalidValue;  // the histogram stays one plane
  if (r->what.kind == kNormal) memcpy(r->what.projection, kIdentityProjection, sizeof(r->what.projection));  // alone
  r->what.kind = kBounded;
  return 0;
}

int cb_renderer_bounded(const cb_renderer *r) {
  return r && (r->what.kind == kBounded || r->what.kind == kAimedBounded) ? 1 : 0;
}

// ---- aimed render (draw_aim.hip; include/cudabrot_amd.h, "Aimed render") ----------------------------------------------

int cb_aim_probe(const cb_fractal_dimensions *dims, const cb_iteration_control *iterations, const double projection[8],
                 const double julia_c[2], int bounded, void *d_states, uint32_t n_threads, uint32_t samples_per_thread,
                 int level, uint32_t *d_mask, cb_counters *d_counters, int kernel_variant, void *stream) {
  const Launch l = {dims, nullptr, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!dims || !iterations || !d_states || !d_mask || dims->w <= 0 || dims->h <= 0 ||
      !plotted_source(&p, bounded ? kAimedBounded : kAimed, projection, julia_c) || !cell_level_ok(level)) {
    return (int) hipErrorInvalidValue;
  }
  cb::AimArgs aa;
  memset(&aa, 0, sizeof(aa));
  bool lockstep = false;
  const int rc = plot_args(l, p.projection, p.julia ? p.julia_c : nullptr, nullptr, !bounded, &aa.p, &lockstep);
  if (rc) return rc;
  aa.bounded = bounded ? 1 : 0;
  aa.mask = d_mask;
  cb::set_grid_level(aa, level);
  const hipError_t e = cb::launch_draw_aim(aa, lockstep, reinterpret_cast<hipStream_t>(stream));
  if (e == hipSuccess) g_last_draw_kernel.store(lockstep ? 31 : 30, std::memory_order_relaxed);  // a refusal names nothing
  return (int) e;
}

int cb_draw_buddhabrot_aimed(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2], int bounded, void *d_states,
                             uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                             int level, const uint32_t *d_cells, uint32_t n_cells, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, bounded ? kAimedBounded : kAimed, projection, julia_c) ||
      !cell_list_ok(level, d_cells, n_cells)) {
    return (int) hipErrorInvalidValue;
  }
  p.cells = {level, const_cast<uint32_t *>(d_cells), n_cells, kernel_variant & kStepBits};  // lent: a launch only reads it
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_aim(cb_renderer *r, int level, uint32_t probe_passes, int dilate, int kernel_variant) {
  if (!r) return (int) hipErrorInvalidValue;
  const bool bounded = r->what.kind == kBounded;
  if (!admits(r, bounded ? kAimedBounded : kAimed) || probe_passes == 0 || dilate < 0 || !cell_level_ok(level)) {
    return (int) hipErrorInvalidValue;
  }
  const double *projection = r->what.kind == kNormal ? kIdentityProjection : r->what.projection;  // alone: the identity
  const double *julia_c = r->what.kind != kNormal && r->what.julia ? r->what.julia_c : nullptr;
  const auto probe = [=](void *d_states, uint32_t samples_per_thread, uint32_t *d_mask) {
    return cb_aim_probe(&r->dims, &r->iterations, projection, julia_c, bounded ? 1 : 0, d_states, r->n_threads,
                        samples_per_thread, level, d_mask, nullptr, kernel_variant, r->stream);
  };
  const int rc = probe_cells(r, level, probe_passes, dilate, probe, CB_ERROR_AIM_EMPTY);
  if (rc) return rc;
  if (r->what.kind == kNormal) memcpy(r->what.projection, kIdentityProjection, sizeof(r->what.projection));
  r->what.kind = bounded ? kAimedBounded : kAimed;
  r->what.cells.step_bits = kernel_variant & kStepBits;
  return 0;
}

int cb_renderer_aim_cells(const cb_renderer *r, uint32_t *n_cells, uint32_t *n_total) {
  if (!r) return (int) hipErrorInvalidValue;
  return renderer_cells(r, r->what.kind == kAimed || r->what.kind == kAimedBounded, n_cells, n_total);
}

int cb_draw_buddhabrot_periods(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2], const uint32_t *d_lut,
                               uint32_t n_entries, double period_eps, void *d_states, uint32_t n_threads,
                               uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, void *stream) {
  const Launch l = {dims, d_hist, iterations, d_states, n_threads, samples_per_thread, d_counters, kernel_variant, stream};
  Plotted p;
  if (!launch_ok(l) || !plotted_source(&p, kPeriodPalette, projection, julia_c)) return (int) hipErrorInvalidValue;
  if (!d_lut || !period_palette_ok(n_entries, period_eps)) return (int) hipErrorInvalidValue;
  p.d_lut = d_lut;
  p.n_entries = n_entries;
  p.period_eps = period_eps;
  return draw_plotted(l, p, nullptr);
}

int cb_renderer_set_period_palette(cb_renderer *r, const uint32_t *lut_host, uint32_t n_entries, double eps) {
  if (!admits(r, kPeriodPalette) || !period_palette_ok(n_entries, eps) || !lut_host_ok(lut_host, n_entries)) {
    return (int) hipErrorInvalidValue;
  }
  const int rc = swap_in_planes(r, 3, lut_host, n_entries, &r->what.d_lut);
  if (rc) return rc;
  if (r->what.kind == kNormal) memcpy(r->what.projection, kIdentityProjection, sizeof(r->what.projection));  // alone
  r->what.n_entries = n_entries;
  r->what.period_eps = eps;
  r->what.kind = kPeriodPalette;
  return 0;
}

int cb_renderer_period_palette(const cb_renderer *r, uint32_t *n_entries, double *eps) {
  if (!r || r->what.kind != kPeriodPalette) return 0;
  if (n_entries) *n_entries = r->what.n_entries;
  if (eps) *eps = r->what.period_eps;
  return 1;
}

int cb_renderer_create(cb_renderer **out, int device, const cb_fractal_dimensions *dims,
                       const cb_iteration_control *iterations, uint64_t seed,
                       uint64_t first_subsequence, uint32_t n_threads) {
  return cb_renderer_create_channels(out, device, dims, iterations, 0, seed, first_subsequence, n_threads);
}

int cb_renderer_create_channels(cb_renderer **out, int device, const cb_fractal_dimensions *dims,
                                const cb_iteration_control *iterations, int n_channels, uint64_t seed,
                                uint64_t first_subsequence, uint32_t n_threads) {
  if (!out || !dims || !iterations || dims->w <= 0 || dims->h <= 0 || n_threads == 0 || n_channels < 0 ||
      n_channels > CB_MAX_CHANNELS) {
    return (int) hipErrorInvalidValue;
  }
  *out = nullptr;
  CB_TRY(hipSetDevice(device));  // cudabrot.cu:155
  cb_renderer *r = new (std::nothrow) cb_renderer;
  if (!r) return (int) hipErrorOutOfMemory;
  memset(r, 0, sizeof(*r));
  r->device = device;
  r->dims = *dims;
  r->iterations = *iterations;
  r->n_channels = n_channels;
  for (int j = 0; j < n_channels; ++j) r->windows[j] = iterations[j];
  r->n_threads = n_threads;
  r->seed = seed;
  r->first_subsequence = first_subsequence;
  const size_t hist_bytes = (size_t) dims->w * (size_t) dims->h * sizeof(cb_pixel) * (size_t) (n_channels ? n_channels : 1);
  hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->flush_stream, hipStreamNonBlocking);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = hipEventCreateWithFlags(&r->draw_done[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->flush_done[k], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipMalloc(&r->d_hist, hist_bytes);                  // cudabrot.cu:168
  if (e == hipSuccess) e = hipMemsetAsync(r->d_hist, 0, hist_bytes, r->stream);  // cudabrot.cu:169
  if (e == hipSuccess) e = hipMalloc(&r->d_states, cb_rng_state_bytes(n_threads));  // :177
  if (e == hipSuccess) e = hipMalloc(&r->d_counters, sizeof(cb_counters));
  if (e == hipSuccess) e = hipMalloc(&r->d_carry, cb_carry_bytes(n_threads));
  if (e == hipSuccess) e = hipMemsetAsync(r->d_carry, 0, cb_carry_bytes(n_threads), r->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r->d_counters, 0, sizeof(cb_counters), r->stream);
  int rc = (int) e;
  if (!rc) rc = cb_initialize_rng(seed, first_subsequence, n_threads, r->d_states, r->stream);
  if (!rc) rc = (int) hipStreamSynchronize(r->stream);  // cudabrot.cu:181
  if (rc) {
    cb_renderer_destroy(r);
    return rc;
  }
  *out = r;
  return 0;
}

namespace {

// 50 samples per thread per reference pass (cudabrot.cu:34,390), at most kRendererPassesPerLaunch passes per launch.
uint32_t max_passes_per_launch() {
  static const uint32_t v = [] {
    const char *e = cb_debug_knob("CUDABROT_AMD_PASSES_PER_LAUNCH");  // experiment knob
    const long n = e ? atol(e) : 0;
    return (n >= 1 && n <= 4096) ? (uint32_t) n : kRendererPassesPerLaunch;
  }();
  return v;
}

// What a renderer allocates on first use, because it depends on the kernel variant: the two scatter
// workspaces (tens of GB on a large canvas -- hipMalloc of that size can take seconds).
void prepare_for_variant(cb_renderer *r, int kernel_variant) {
  if ((kernel_variant & ~kVariantFlags) == CB_KERNEL_TIMED && cb_debug_knob("CUDABROT_AMD_WAVE_DUMP") &&
      !g_wave_dump) {
    const size_t bytes = (size_t) cb::draw_wave_count(r->n_threads) * 8 * sizeof(unsigned long long);
    if (hipMalloc(&g_wave_dump, bytes) != hipSuccess || hipMemset(g_wave_dump, 0, bytes) != hipSuccess) {
      g_wave_dump = nullptr;
    }
  }
  if (!r->workspace_tried && r->what.kind == kNormal &&  // the focus and plotted kernels add directly
      (kernel_variant & ~kVariantFlags) != CB_KERNEL_SIMPLE &&
      (kernel_variant & CB_KERNEL_FLAG_ANTI) == 0 &&  // the anti kernels add directly
      cb_debug_knob("CUDABROT_AMD_NO_WORKSPACE") == nullptr) {
    // scatter workspace for the largest launch render_passes makes; on any failure: direct atomics
    r->workspace_tried = 1;
    size_t want = cb_scatter_workspace_bytes_channels(&r->dims, r->n_channels > 0 ? r->n_channels : 1, r->n_threads,
                                                      max_passes_per_launch() * CB_SAMPLES_PER_THREAD);
    size_t free_b = 0, total_b = 0;
    if (want && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      if (want > free_b / 4) want = free_b / 4;
      if (hipMalloc(&r->d_workspace[0], want) == hipSuccess &&
          hipMalloc(&r->d_workspace[1], want) == hipSuccess) {
        r->workspace_bytes = want;
      } else {
        (void) hipGetLastError();
        (void) hipFree(r->d_workspace[0]);
        (void) hipFree(r->d_workspace[1]);
        r->d_workspace[0] = r->d_workspace[1] = nullptr;
      }
    }
  }
}

}  // namespace

int cb_renderer_prepare(cb_renderer *r, int kernel_variant) {
  if (!r || !variant_ok(r->what, kernel_variant)) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  prepare_for_variant(r, kernel_variant);
  return (int) hipDeviceSynchronize();
}

int cb_renderer_render_passes(cb_renderer *r, uint32_t passes, int kernel_variant) {
  if (!r) return (int) hipErrorInvalidValue;
  if ((kernel_variant & (CB_KERNEL_POWER_MASK | CB_KERNEL_FORMULA_MASK)) != 0 && !is_plotted(r->what.kind)) {
    return (int) hipErrorInvalidValue;  // a degree, a formula: on a projected, Julia or palette renderer only
  }
  if (!variant_ok(r->what, kernel_variant)) return (int) hipErrorInvalidValue;  // (a Phoenix renderer)
  CB_TRY(hipSetDevice(r->device));
  const uint32_t max_passes_per_launch = ::max_passes_per_launch();
  prepare_for_variant(r, kernel_variant);
  if (passes > 0) r->rendered = true;
  if (r->carry_pending && r->carry_variant != kernel_variant) {
    int rc = finish(r);  // a different kernel variant cannot take over the carried work
    if (rc) return rc;
  }
  while (passes > 0) {
    const uint32_t now = passes < max_passes_per_launch ? passes : max_passes_per_launch;
    int rc = enqueue_launch(r, now, kernel_variant);
    if (rc) return rc;
    passes -= now;
  }
  // The draw launches are complete when this returns (the fence at the end); the scatter of the last one may
  // still be running on its own stream, so that the first draw launch of the next call starts beside it --
  // a caller that renders in batches (the binary: every ~0.2 s) keeps the pipeline of enqueue_launch going
  // across calls.  Everything that reads the histogram or the counters goes through finish(), which completes
  // the carried orbits and waits for both streams.
  if (g_wave_dump) {  // diagnostic: write the per-wave records of the last launch
    (void) hipStreamSynchronize(r->stream);
    const size_t n = (size_t) cb::draw_wave_count(r->n_threads) * 8;
    std::vector<unsigned long long> host(n);
    if (hipMemcpy(host.data(), g_wave_dump, n * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      if (FILE *f = fopen(cb_debug_knob("CUDABROT_AMD_WAVE_DUMP"), "wb")) {
        fwrite(host.data(), 8, n, f);
        fclose(f);
      }
    }
    (void) hipFree(g_wave_dump);
    g_wave_dump = nullptr;
  }
  return (int) hipStreamSynchronize(r->stream);  // cudabrot.cu:487
}

int cb_renderer_finish(cb_renderer *r) {
  if (!r) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  return finish(r);
}

int cb_renderer_read_histogram(cb_renderer *r, cb_pixel *host_out) {
  if (!r || !host_out) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  const size_t bytes = (size_t) r->dims.w * (size_t) r->dims.h * sizeof(cb_pixel) * renderer_planes(r);
  CB_TRY(hipMemcpyAsync(host_out, r->d_hist, bytes, hipMemcpyDeviceToHost, r->stream));
  return (int) hipStreamSynchronize(r->stream);
}

int cb_renderer_grayscale_image(cb_renderer *r, double gamma, int mode, uint16_t *host_gray_be,
                                uint64_t *max_out, double *scale_out) {
  return cb_renderer_grayscale_plane(r, 0, gamma, mode, host_gray_be, max_out, scale_out);
}

int cb_renderer_grayscale_plane(cb_renderer *r, int plane, double gamma, int mode, uint16_t *host_gray_be,
                                uint64_t *max_out, double *scale_out) {
  if (!r || !host_gray_be || plane < 0 || (size_t) plane >= renderer_planes(r)) {
    return (int) hipErrorInvalidValue;
  }
  return gray_image(r, (size_t) plane, r->dims.h, gamma, mode, host_gray_be, max_out, scale_out);
}

namespace {

// The image of three planes R, G, B ("Palette render", Image).
int three_plane_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                      double *scale_out) {
  if (r->dims.h > 0x7fffffff / 3) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  const size_t n = (size_t) r->dims.w * (size_t) r->dims.h;
  uint16_t *d_planes = nullptr, *d_rgb = nullptr;
  int rc = (int) hipMalloc(reinterpret_cast<void **>(&d_planes), 3 * n * sizeof(uint16_t));
  if (rc == 0) rc = (int) hipMalloc(reinterpret_cast<void **>(&d_rgb), 3 * n * sizeof(uint16_t));
  // the three planes as one w x 3h image: one maximum for all of them
  // (and one group for the density filter: a colour pixel is smoothed as one thing)
  if (rc == 0) rc = tone_map_rows(r, r->d_hist, 3 * r->dims.h, r->dims.h, 3, gamma, tone_mode, d_planes, max_out, scale_out);
  if (rc == 0) {
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(interleave_planes_kernel, dim3((uint32_t) (blocks < 4096 ? blocks : 4096)), dim3(256), 0, r->stream,
                       d_planes, n, d_rgb);
    rc = (int) hipGetLastError();
  }
  if (rc == 0) rc = (int) hipMemcpyAsync(host_rgb_be, d_rgb, 3 * n * sizeof(uint16_t), hipMemcpyDeviceToHost, r->stream);
  if (rc == 0) rc = (int) hipStreamSynchronize(r->stream);
  (void) hipFree(d_planes);
  (void) hipFree(d_rgb);
  return rc;
}

// The image of a renderer of `kind` and no other, all its planes under one maximum: what the four cb_renderer_*_image calls
// of the plotted kinds do.
int kind_image(cb_renderer *r, Kind kind, double gamma, int tone_mode, uint16_t *host_be, uint64_t *max_out,
               double *scale_out) {
  if (!r || r->what.kind != kind || !host_be) return (int) hipErrorInvalidValue;
  const KindRow row = kind_row(r->what);
  switch (row.image) {
    case kImageRgb: return three_plane_image(r, gamma, tone_mode, host_be, max_out, scale_out);
    case kImageSingle:
    case kImageStacked:  // one w x N*h image (N * h fits an int: depth_ok, frames_ok)
      return gray_image(r, 0, (int) row.planes * r->dims.h, gamma, tone_mode, host_be, max_out, scale_out);
  }
  return (int) hipErrorInvalidValue;
}

}  // namespace

int cb_renderer_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                              double *scale_out) {
  return kind_image(r, kPalette, gamma, tone_mode, host_rgb_be, max_out, scale_out);
}

int cb_renderer_depth_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                                    double *scale_out) {
  return kind_image(r, kDepthPalette, gamma, tone_mode, host_rgb_be, max_out, scale_out);
}

int cb_renderer_period_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                                     double *scale_out) {
  return kind_image(r, kPeriodPalette, gamma, tone_mode, host_rgb_be, max_out, scale_out);
}

int cb_renderer_depth_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_gray_be, uint64_t *max_out,
                            double *scale_out) {
  return kind_image(r, kDepth, gamma, tone_mode, host_gray_be, max_out, scale_out);
}

int cb_renderer_frames_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_gray_be, uint64_t *max_out,
                             double *scale_out) {
  return kind_image(r, kFrames, gamma, tone_mode, host_gray_be, max_out, scale_out);
}

int cb_renderer_color_image(cb_renderer *r, const int planes[3], double gamma, int tone_mode,
                            const cb_color_params *p, uint16_t *host_rgb_be, uint16_t levels[6]) {
  if (!r || !planes || !host_rgb_be || !cb::color_params_ok(p)) return (int) hipErrorInvalidValue;
  if (r->white_clip != 0.0) return (int) hipErrorInvalidValue;  // the colour stage has a stretch of its own ("White clip")
  if (r->density_radius != 0) return (int) hipErrorInvalidValue;  // and works on 16-bit planes ("Density filter")
  if (r->equalize) return (int) hipErrorInvalidValue;             // its stretch again ("Equalised image")
  if (r->local_tiles_x != 0) return (int) hipErrorInvalidValue;   // and again ("Locally equalised image")
  const size_t n = (size_t) r->dims.w * (size_t) r->dims.h;
  const cb_pixel *src[3];
  for (int j = 0; j < 3; ++j) {
    if (planes[j] < 0 || (size_t) planes[j] >= renderer_planes(r)) return (int) hipErrorInvalidValue;
    src[j] = r->d_hist + (size_t) planes[j] * n;
  }
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  const size_t bytes = 3 * n * sizeof(uint16_t);
  uint16_t *d_rgb = nullptr;
  CB_TRY(hipMalloc(reinterpret_cast<void **>(&d_rgb), bytes));
  int rc = cb_compose_color_device(src, r->dims.w, r->dims.h, gamma, tone_mode, p, d_rgb, levels, r->stream);
  if (rc == 0) rc = (int) hipMemcpyAsync(host_rgb_be, d_rgb, bytes, hipMemcpyDeviceToHost, r->stream);
  if (rc == 0) rc = (int) hipStreamSynchronize(r->stream);
  (void) hipFree(d_rgb);
  return rc;
}

int cb_renderer_set_white_clip(cb_renderer *r, double percent) {
  if (!r || !cb_white_clip_ok(percent)) return (int) hipErrorInvalidValue;
  if (percent != 0.0 && r->equalize) return (int) hipErrorInvalidValue;  // one exposure at a time ("Equalised image")
  if (percent != 0.0 && r->local_tiles_x != 0) return (int) hipErrorInvalidValue;  // ("Locally equalised image")
  r->white_clip = percent;
  if (!r->equalize && r->local_tiles_x == 0) r->last_exposed = {0, 0, 0, 0, 0, 0};  // (an equalised renderer keeps what it found: nothing changed)
  return 0;
}

int cb_renderer_white_clip(const cb_renderer *r, double *percent_out) {
  if (!r || !percent_out) return (int) hipErrorInvalidValue;
  *percent_out = r->white_clip;
  return 0;
}

int cb_renderer_set_density_filter(cb_renderer *r, int radius, double alpha, uint64_t n0) {
  if (!r) return (int) hipErrorInvalidValue;
  uint64_t table[CB_DENSITY_MAX_RADIUS + 1] = {};
  if (radius != 0 && cb_density_thresholds(radius, alpha, n0, table) != 0) return (int) hipErrorInvalidValue;
  r->density_radius = radius;
  r->density_alpha = radius ? alpha : 0.0;
  r->density_n0 = radius ? n0 : 0;
  memcpy(r->density_thresholds, table, sizeof(table));
  return 0;
}

int cb_renderer_density_filter(const cb_renderer *r, int *radius_out, double *alpha_out, uint64_t *n0_out) {
  if (!r || !radius_out || !alpha_out || !n0_out) return (int) hipErrorInvalidValue;
  *radius_out = r->density_radius;
  *alpha_out = r->density_alpha;
  *n0_out = r->density_n0;
  return 0;
}

int cb_renderer_last_white(const cb_renderer *r, uint64_t *white_out, uint64_t *lit_out, uint64_t *clipped_out) {
  if (!r || !white_out || !lit_out || !clipped_out) return (int) hipErrorInvalidValue;
  *white_out = r->last_exposed.white;
  *lit_out = (r->equalize || r->local_tiles_x != 0) ? 0 : r->last_exposed.lit;  // (an equalised image counts its lit pixels too)
  *clipped_out = r->last_exposed.clipped;
  return 0;
}

int cb_renderer_set_equalize(cb_renderer *r, int on) {
  if (!r || (on != 0 && (r->white_clip != 0.0 || r->local_tiles_x != 0))) return (int) hipErrorInvalidValue;
  r->equalize = on != 0;
  if (r->white_clip == 0.0 && r->local_tiles_x == 0) r->last_exposed = {0, 0, 0, 0, 0, 0};  // (likewise a clipped one)
  return 0;
}

int cb_renderer_equalize(const cb_renderer *r) { return (r && r->equalize) ? 1 : 0; }

int cb_renderer_last_equalize(const cb_renderer *r, uint64_t *lit_out, uint64_t *keys_out, uint64_t *levels_out) {
  if (!r || !lit_out || !keys_out || !levels_out) return (int) hipErrorInvalidValue;
  *lit_out = r->equalize ? r->last_exposed.lit : 0;  // (so does a clipped one)
  *keys_out = r->last_exposed.keys;
  *levels_out = r->last_exposed.levels;
  return 0;
}

int cb_renderer_set_local_equalize(cb_renderer *r, int tx, int ty, uint32_t clip_q) {
  if (!r) return (int) hipErrorInvalidValue;
  if (tx != 0) {  // one exposure at a time
    if (r->white_clip != 0.0 || r->equalize || !cb_local_equalize_ok(r->dims.w, r->dims.h, 1, tx, ty, clip_q)) {
      return (int) hipErrorInvalidValue;
    }
  }
  r->local_tiles_x = tx;
  r->local_tiles_y = tx ? ty : 0;
  r->local_clip_q = tx ? clip_q : 0;
  if (r->white_clip == 0.0 && !r->equalize) r->last_exposed = {0, 0, 0, 0, 0, 0};  // (those keep what they found)
  return 0;
}

int cb_renderer_local_equalize(const cb_renderer *r, int *tx_out, int *ty_out, uint32_t *clip_q_out) {
  if (!r || !tx_out || !ty_out || !clip_q_out) return (int) hipErrorInvalidValue;
  *tx_out = r->local_tiles_x;
  *ty_out = r->local_tiles_y;
  *clip_q_out = r->local_clip_q;
  return 0;
}

int cb_renderer_last_local_equalize(const cb_renderer *r, uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out) {
  if (!r || !lit_out || !lit_tiles_out || !moved_out) return (int) hipErrorInvalidValue;
  *lit_out = r->local_tiles_x != 0 ? r->last_exposed.lit : 0;
  *lit_tiles_out = r->last_exposed.lit_tiles;
  *moved_out = r->last_exposed.moved;
  return 0;
}

int cb_renderer_write_histogram(cb_renderer *r, const cb_pixel *host_in) {
  if (!r || !host_in) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  const size_t bytes = (size_t) r->dims.w * (size_t) r->dims.h * sizeof(cb_pixel) * renderer_planes(r);
  CB_TRY(hipMemcpyAsync(r->d_hist, host_in, bytes, hipMemcpyHostToDevice, r->stream));
  return (int) hipStreamSynchronize(r->stream);
}

int cb_renderer_read_counters(cb_renderer *r, cb_counters *host_out) {
  if (!r || !host_out) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc && rc != CB_ERROR_KERNEL_INVARIANT) return rc;  // the counters are how a caller reads the status
  }
  CB_TRY(hipMemcpyAsync(host_out, r->d_counters, sizeof(cb_counters), hipMemcpyDeviceToHost,
                        r->stream));
  return (int) hipStreamSynchronize(r->stream);
}

int cb_renderer_read_rng_states(cb_renderer *r, void *host_out) {
  if (!r || !host_out) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);  // afterwards no orbit is in flight: states + histogram are a complete checkpoint
    if (rc) return rc;
  }
  CB_TRY(hipMemcpyAsync(host_out, r->d_states, cb_rng_state_bytes(r->n_threads), hipMemcpyDeviceToHost,
                        r->stream));
  return (int) hipStreamSynchronize(r->stream);
}

int cb_renderer_write_rng_states(cb_renderer *r, const void *host_in) {
  if (!r || !host_in) return (int) hipErrorInvalidValue;
  CB_TRY(hipSetDevice(r->device));
  {
    int rc = finish(r);
    if (rc) return rc;
  }
  CB_TRY(hipMemcpyAsync(r->d_states, host_in, cb_rng_state_bytes(r->n_threads), hipMemcpyHostToDevice,
                        r->stream));
  return (int) hipStreamSynchronize(r->stream);
}

cb_pixel *cb_renderer_device_histogram(cb_renderer *r) { return r ? r->d_hist : nullptr; }

void cb_renderer_destroy(cb_renderer *r) {
  if (!r) return;
  (void) hipSetDevice(r->device);
  if (r->stream) (void) hipStreamSynchronize(r->stream);
  if (r->flush_stream) (void) hipStreamSynchronize(r->flush_stream);
  release_communicators_with(r->device);  // (cached by cb_renderers_reduce for a set this renderer may belong to)
  (void) hipFree(r->d_hist);
  (void) hipFree(r->d_states);
  (void) hipFree(r->d_counters);
  (void) hipFree(r->d_carry);
  (void) hipFree(r->what.cells.d_cells);
  (void) hipFree(const_cast<uint32_t *>(r->what.d_lut));
  (void) hipFree(const_cast<double *>(r->what.d_frames));
  delete r->frames;
  (void) hipFree(r->d_workspace[0]);
  (void) hipFree(r->d_workspace[1]);
  for (int k = 0; k < 2; ++k) {
    if (r->draw_done[k]) (void) hipEventDestroy(r->draw_done[k]);
    if (r->flush_done[k]) (void) hipEventDestroy(r->flush_done[k]);
  }
  if (r->stream) (void) hipStreamDestroy(r->stream);
  if (r->flush_stream) (void) hipStreamDestroy(r->flush_stream);
  delete r;
}

// The one exchange of the multi-GPU path: renderers[0] += renderers[1..n).  Renderers on
// n distinct devices: one ncclReduce(ncclUint64, ncclSum, root 0) over xGMI.  RCCL is loaded on first
// use (dlopen), so single-GPU users of the library never touch it.  Renderers that all share one device
// (a rehearsal of the sharded path on a one-GPU box): an add kernel.
int cb_renderers_reduce(cb_renderer *const *renderers, int n) {
  if (!renderers || n < 1) return (int) hipErrorInvalidValue;
  for (int k = 0; k < n; ++k) {
    cb_renderer *r = renderers[k];
    if (!r || r->dims.w != renderers[0]->dims.w || r->dims.h != renderers[0]->dims.h ||
        r->n_channels != renderers[0]->n_channels ||
        (r->what.kind == kPalette) != (renderers[0]->what.kind == kPalette) ||
        (r->what.kind == kDepthPalette) != (renderers[0]->what.kind == kDepthPalette) ||
        (r->what.kind == kPeriodPalette) != (renderers[0]->what.kind == kPeriodPalette) ||
        renderer_planes(r) != renderer_planes(renderers[0])) {
      return (int) hipErrorInvalidValue;
    }
    CB_TRY(hipSetDevice(r->device));
    const int rc = finish(r);
    if (rc) return rc;
  }
  cb_renderer *root = renderers[0];
  const size_t count = (size_t) root->dims.w * (size_t) root->dims.h * renderer_planes(root);
  if (n == 1) {
    // CUDABROT_AMD_FORCE_RCCL=1 (test knob): a reduce over one rank, to exercise the RCCL calls where
    // only one device exists
    return cb_debug_knob("CUDABROT_AMD_FORCE_RCCL") ? rccl_reduce_to_root(renderers, 1, count) : 0;
  }
  bool same = true, distinct = true;
  for (int a = 0; a < n; ++a) {
    if (renderers[a]->device != root->device) same = false;
    for (int b = a + 1; b < n; ++b) {
      if (renderers[a]->device == renderers[b]->device) distinct = false;
    }
  }
  if (same) {
    CB_TRY(hipSetDevice(root->device));
    for (int k = 1; k < n; ++k) {
      hipLaunchKernelGGL(add_histogram_kernel, dim3(256 * 8), dim3(256), 0, root->stream,
                         reinterpret_cast<unsigned long long *>(root->d_hist),
                         reinterpret_cast<const unsigned long long *>(renderers[k]->d_hist), count);
      CB_TRY(hipGetLastError());
    }
    return (int) hipStreamSynchronize(root->stream);
  }
  if (!distinct) return (int) hipErrorInvalidValue;
  return rccl_reduce_to_root(renderers, n, count);
}

}  // extern "C"
