// cli_args.h -- the `cudabrot` command line: what it sets (Settings) and its parser (cli_args.cpp).  Host code over
// include/cudabrot_amd.h alone: no device is touched before the run (cli_main.cpp) starts.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/cudabrot_amd.h"

namespace cb {

// --sweep X,Y:DEG0:DEG1:F as given: the two axes (columns of P), the angles and the number of frames.
struct Sweep {
  int axis_x, axis_y;
  double deg0, deg1;
  int frames;
};

// --focus / --aim and their three value flags: whether samples come from a probed cell list, and how the list is made.
struct CellFlags {
  bool on = false;
  int level = 8;     // --*-level: cells of side 2^-L
  long probe = 64;   // --*-probe: reference passes of the probe
  int dilate = 1;    // --*-dilate: cells the probe's mask is widened by
};

// --density-filter R[:ALPHA[:N0]] as given, the defaults where a part is left out; radius 0: no flag.
struct DensityFilter {
  int radius = 0;
  double alpha = 0.5;
  uint64_t n0 = 1;
};

// --local-equalize TX[xTY][:CLIP] as given: TY = TX and CLIP = 4 where left out, the clip in 1/256ths; tx 0: no flag.
struct LocalEqualize {
  int tx = 0, ty = 0;
  uint32_t clip_q = 0;
};

// A list of colour stops, K:RRGGBB[,K:RRGGBB...], as --palette, --depth-palette and --period-palette give one; none: no flag.
struct Stops {
  int n = 0;
  cb_palette_stop at[CB_PALETTE_MAX_STOPS] = {};
  bool given() const { return n > 0; }
};

// What a run renders into and writes, by the flag that decides it (Settings::output): the renderer's image of each is
// cli_main.cpp's table.
enum class Sink { kGray, kChannels, kDepth, kSweep, kPalette, kDepthPalette, kPeriodPalette };
// The four shapes of the output: one gray plane, one PGM; --channel planes, one PGM each; N planes as N PGMs back to back
// in one file; three planes as one PPM.
enum class Shape { kGray, kChannels, kStack, kColor };
struct Output {
  Sink sink;
  Shape shape;
  int planes;  // of counters, each of the canvas's size
};

struct Settings {
  int device = 0;                                   // -d
  const char *output_image = "output.pgm";          // -o   (cudabrot.cu:26,764)
  const char *inprogress_file = nullptr;            // -s
  double seconds_to_run = 10.0;                     // -t   (cudabrot.cu:769)
  double gamma_correction = 1.0;                    // -g   (cudabrot.cu:770)
  cb_iteration_control iterations = {100, 20};      // -m -c (cudabrot.cu:765-766)
  cb_fractal_dimensions canvas = {1000, 1000, -2.0, -2.0, 2.0, 2.0, 0.0, 0.0};  // cudabrot.cu:533-538
  long fixed_passes = -1;                           // --passes (extension; <0: run by the clock)
  int kernel_variant = CB_KERNEL_DEFAULT;           // --kernel (extension)
  bool print_stats = false;                         // --stats  (extension)
  bool burning_ship = false;                        // --burning-ship (extension; cudabrot.cu:15-17)
  bool anti = false;                                // --anti (extension): the anti-Buddhabrot, CB_KERNEL_FLAG_ANTI
  int gpus = 1;                                     // --gpus N (extension): devices -d .. -d + N - 1
  // --channel MAX:MIN:FILE (extension, repeatable): fused multi-channel render, one image per window
  int n_channels = 0;
  cb_iteration_control channel_window[CB_MAX_CHANNELS] = {};
  std::string channel_file[CB_MAX_CHANNELS];
  uint64_t seed = CB_DEFAULT_RNG_SEED;              // --seed (extension; cudabrot.cu:37)
  const char *rng_state_file = nullptr;             // --rng-state (extension): true-resume sidecar
  bool raw_state = false;                           // --state-format raw (extension): -s as the reference's bare buffer
  int tone_mode = CB_TONE_AUTO;                     // --tonemap (extension): device table / thresholds
  bool host_tonemap = false;                        //   ... or the reference's host loop
  // --color FILE (extension): the three --channel planes composed into one RGB image; --compose, --hue-shift,
  // --color-stretch B:W set its cb_color_params (defaults: rgb, 0, ImageMagick's -normalize 2:1)
  const char *color_file = nullptr;
  cb_color_params color = {CB_COMPOSE_RGB, 2.0, 1.0, 0.0};
  // --focus (extension): samples drawn only from the cells a probe found to reach the canvas (cb_renderer_set_focus)
  CellFlags focus;
  // --project / --plane / --rotate (extensions): the plotted plane, P[2][4] over (zr, zi, cr, ci) (cb_renderer_set_projection)
  bool project_given = false, plane_given = false, rotate_given = false;
  double projection[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  // --power D (extension): the Multibrot step z^D + c, CB_KERNEL_POWER(D); makes the run a projected one (the identity
  // unless a plane is given)
  int power = 0;
  // --julia RE,IM (extension): the Buddhabrot of the Julia set of c = RE + IM i (cb_renderer_set_julia); makes the run a
  // projected one as --power does
  bool julia = false;
  double julia_c[2] = {0.0, 0.0};
  // --palette K:RRGGBB[,K:RRGGBB...] (extension): the colour stops of a palette render (cb_palette_from_stops,
  // cb_renderer_set_palette); makes the run a projected one as --power does
  Stops palette_stops;
  bool palette() const { return palette_stops.given(); }
  // --formula NAME (extension): a formula step, CB_KERNEL_FORMULA(code); makes the run a projected one as --power does
  int formula = 0;
  const char *formula_name = nullptr;
  bool projected() const {
    return project_given || plane_given || rotate_given || power != 0 || julia || palette() || formula != 0;
  }
  // --depth ROW:MIN:MAX[:N] (extension): the set sliced along a third row into N planes (cb_renderer_set_depth); makes the
  // run a projected one as --power does, but is no part of projected(): its refusals are a row of their own, behind the
  // projection's
  bool depth_given = false;
  cb_depth depth = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0};
  bool plotted() const { return projected() || depth_given || sweep_given || phoenix || bounded || aim.on; }
  // --depth-palette K:RRGGBB[,K:RRGGBB...] (extension): the colour stops of a depth-palette render, K a slice index
  // (cb_palette_from_stops with --depth's N entries, cb_renderer_set_depth_palette); needs --depth, whose N planes become
  // three
  Stops depth_palette_stops;
  bool depth_palette() const { return depth_palette_stops.given(); }
  // --sweep X,Y:DEG0:DEG1:F (extension): F frames of the plane rotated in (X, Y), one orbit pass (cb_frames_from_sweep,
  // cb_renderer_set_frames); makes the run a projected one as --depth does, with a last refusal row of its own.  The base
  // is `projection` as it stands when the flags have been read: the sweep is applied last, at most once.
  bool sweep_given = false;
  Sweep sweep = {0, 1, 0.0, 0.0, 0};
  // --phoenix RE,IM (extension): the Phoenix step with p = RE + IM i (cb_renderer_set_phoenix); makes the run a projected
  // one as --depth does, with a last refusal row of its own; combines with --julia
  bool phoenix = false;
  double phoenix_p[2] = {0.0, 0.0};
  // --bounded (extension): the orbits that never escape, on the plotted path (cb_renderer_set_bounded); makes the run a
  // projected one as --depth does, with a refusal row of its own; combines with every plane, step and --julia.  -c is not
  // read, as under --anti
  bool bounded = false;
  // --period-palette K:RRGGBB[,K:RRGGBB...] (extension): the colour stops of a period-palette render, K a period from 0 to
  // CB_PERIOD_MAX_ENTRIES - 1 (cb_palette_from_stops with the largest K + 1 entries, at least 2,
  // cb_renderer_set_period_palette); needs --bounded, whose one plane becomes three.  --period-eps X: the tolerance of the
  // return test, which needs --period-palette
  Stops period_stops;
  bool period_palette() const { return period_stops.given(); }
  uint32_t period_entries() const {  // the largest K given + 1, and at least 2
    const int last = period_palette() ? period_stops.at[period_stops.n - 1].k : 0;
    return last < 1 ? 2u : (uint32_t) last + 1u;
  }
  bool period_eps_given = false;
  double period_eps = 0x1p-66;
  // --aim (extension): a plotted render -- projected or Julia, under any of their steps, or --bounded -- whose samples are
  // drawn only from the cells of the sample plane a probe found to reach the canvas (cb_renderer_set_aim); makes the run a
  // projected one as --depth does (alone: the identity), with a first refusal row of its own
  CellFlags aim;
  // --white-clip P (extension): every image of the run exposed against a percentile of its counters instead of their
  // maximum (include/cudabrot_amd.h, "White clip"; cb_renderer_set_white_clip); 0, the default, is off
  double white_clip = 0.0;
  // --density-filter R[:ALPHA[:N0]] (extension): every image of the run made from counters smoothed with a radius that
  // falls as the count rises (include/cudabrot_amd.h, "Density filter"; cb_renderer_set_density_filter); radius 0, the
  // default, is off
  DensityFilter density;
  // --equalize (extension): every image of the run exposed by the rank of its counters among the lit ones instead of by
  // their size (include/cudabrot_amd.h, "Equalised image"; cb_renderer_set_equalize)
  bool equalize = false;
  // --local-equalize TX[xTY][:CLIP] (extension): every image of the run exposed by the rank of its counters within the
  // tiles of a grid, blended between the tile centres (include/cudabrot_amd.h, "Locally equalised image";
  // cb_renderer_set_local_equalize); tx 0, the default, is off
  LocalEqualize local_equalize;
  // The one place that says what the flags above make of the output: a palette of any kind turns its render's planes into
  // three and the file into a PPM, so it goes before the render it colours; --depth and --sweep stack their planes;
  // --channel has an image per plane.  The refusal table lets no two of the renders meet.
  Output output() const {
    if (depth_palette()) return {Sink::kDepthPalette, Shape::kColor, 3};
    if (period_palette()) return {Sink::kPeriodPalette, Shape::kColor, 3};
    if (palette()) return {Sink::kPalette, Shape::kColor, 3};
    if (depth_given) return {Sink::kDepth, Shape::kStack, depth.slices};
    if (sweep_given) return {Sink::kSweep, Shape::kStack, sweep.frames};
    if (n_channels > 0) return {Sink::kChannels, Shape::kChannels, n_channels};
    return {Sink::kGray, Shape::kGray, 1};
  }
};

// argv -> Settings, with the reference's messages (cudabrot.cu:625-754).  A command line that is refused -- --help, an
// unknown flag, a bad value, a combination the renders do not support -- ends the process here: its message and the
// usage text on stdout, exit 0.
Settings parse_arguments(int argc, char **argv);

}  // namespace cb
