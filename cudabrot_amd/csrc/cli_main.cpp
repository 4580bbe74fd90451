// cli_main.cpp -- `cudabrot`: command-line drop-in for the reference binary.
//
// The process boundary IS the reference's public interface: argv in, stdout text,
// exit code, a 16-bit PGM and the raw -s buffer out.  This file and cli_args.cpp reproduce that contract
// (cudabrot.cu:579-791: messages, usage -> exit 0, errors on stdout -> exit 1) on top of the C ABI in
// include/cudabrot_amd.h: the parser there (flags :662-754), the run of what it returns here.  Rendering is done
// by the hand-written gfx950 kernels only: there is no CPU fallback, without a usable GPU the program prints the
// reference's error line and exits 1.
//
// Observable differences, all deliberate:
//  * the -s buffer holds 64-bit counters behind a 32-byte header that names its own shape (magic, w, h, planes,
//    counter width), so a file of another canvas can never be mistaken for this one's; a reference-format
//    file (exactly w*h*4 bytes of uint32, no header) is accepted on load, announced, and widened;
//  * reference passes (512*512 threads x 50 samples) are fused into launches of about 0.2 s, so -t and
//    Ctrl+C act at launch granularity; the printed pass count still counts reference-sized passes;
//  * extension flags, which the reference answers with its usage text: they are listed where they are parsed, in the
//    flag table of cli_args.cpp.
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cudabrot_amd.h"
#include "cli_args.h"
#include "state_files.h"

namespace {

using cb::Settings;

volatile sig_atomic_t g_quit_requested = 0;

// The renderer's image of all the planes of a sink at once, by cb::Sink; none: plane by plane, cb_renderer_grayscale_plane.
using ImageCall = int (*)(cb_renderer *, double, int, uint16_t *, uint64_t *, double *);
constexpr ImageCall kImageOf[] = {
    nullptr,                           // Sink::kGray
    nullptr,                           // Sink::kChannels
    cb_renderer_depth_image,           // Sink::kDepth
    cb_renderer_frames_image,          // Sink::kSweep
    cb_renderer_palette_image,         // Sink::kPalette
    cb_renderer_depth_palette_image,   // Sink::kDepthPalette
    cb_renderer_period_palette_image,  // Sink::kPeriodPalette
};
static_assert(sizeof(kImageOf) / sizeof(kImageOf[0]) == (size_t) cb::Sink::kPeriodPalette + 1, "one row per sink");

// The opening of a --stats line that states a list of stops, {"KEY": [[k, "rrggbb"], ...] -- the caller closes the object.
void print_stops(const char *key, const cb::Stops &stops) {
  fprintf(stderr, "{\"%s\": [", key);
  for (int j = 0; j < stops.n; ++j) {
    const cb_palette_stop &stop = stops.at[j];
    fprintf(stderr, "%s[%d, \"%02x%02x%02x\"]", j ? ", " : "", stop.k, stop.r, stop.g, stop.b);
  }
  fprintf(stderr, "]");
}

// ---- the run -------------------------------------------------------------------------------------

double wall_seconds() {  // cudabrot.cu:122-129
  struct timespec ts;
  if (clock_gettime(CLOCK_REALTIME, &ts) != 0) {
    printf("Error getting time.\n");
    exit(1);
  }
  return (double) ts.tv_sec + (double) ts.tv_nsec / 1e9;
}

class Run {
 public:
  explicit Run(const Settings &s) : cfg_(s), out_(s.output()) {}
  ~Run() { release(); }

  int execute() {
    int max_iterations = cfg_.iterations.max_escape_iterations;
    for (int j = 0; j < cfg_.n_channels; ++j) {
      if (j == 0 || cfg_.channel_window[j].max_escape_iterations > max_iterations) {
        max_iterations = cfg_.channel_window[j].max_escape_iterations;
      }
    }
    printf("Creating %dx%d image, %d max iterations.\n", cfg_.canvas.w, cfg_.canvas.h,
           max_iterations);  // cudabrot.cu:779-780
    printf("Calculating image...\n");
    if (cfg_.sweep_given) {  // the matrices of the frames, from the plane as every other flag has left it
      const cb::Sweep &w = cfg_.sweep;
      frames_.resize(8 * (size_t) w.frames);
      sweep_angles_.resize((size_t) w.frames);
      if (cb_frames_from_sweep(cfg_.projection, w.axis_x, w.axis_y, w.deg0, w.deg1, w.frames, frames_.data(),
                               sweep_angles_.data()) != 0) {
        printf("Invalid sweep: the angles of its frames are not finite.\n");
        return 1;
      }
    }
    if (cfg_.plotted() && cfg_.print_stats) {  // the matrix defines the run: printed before any device is touched
      const double *p = cfg_.projection;
      fprintf(stderr, "{\"projection\": [\"%a\", \"%a\", \"%a\", \"%a\", \"%a\", \"%a\", \"%a\", \"%a\"]}\n", p[0], p[1], p[2],
              p[3], p[4], p[5], p[6], p[7]);
      if (cfg_.power != 0) fprintf(stderr, "{\"power\": %d}\n", cfg_.power);  // the step: it defines the run as well
      if (cfg_.formula != 0) fprintf(stderr, "{\"formula\": \"%s\"}\n", cfg_.formula_name);  // or this step
      if (cfg_.julia) fprintf(stderr, "{\"julia\": [\"%a\", \"%a\"]}\n", cfg_.julia_c[0], cfg_.julia_c[1]);  // and so does c
      if (cfg_.phoenix) fprintf(stderr, "{\"phoenix\": [\"%a\", \"%a\"]}\n", cfg_.phoenix_p[0], cfg_.phoenix_p[1]);  // and p
      if (cfg_.bounded) fprintf(stderr, "{\"bounded\": true}\n");  // and which orbits are plotted
      if (cfg_.aim.on) {  // and where the samples come from: the list is a function of these and of the lines above
        fprintf(stderr, "{\"aim\": {\"level\": %d, \"probe\": %ld, \"dilate\": %d}}\n", cfg_.aim.level, cfg_.aim.probe,
                cfg_.aim.dilate);
      }
      if (cfg_.period_palette()) {  // and the colours of their periods, with the tolerance of the return test
        print_stops("period_palette", cfg_.period_stops);
        fprintf(stderr, ", \"period_eps\": \"%a\"}\n", cfg_.period_eps);
      }
      if (cfg_.depth_given) {  // and the third row with its window
        const cb_depth &d = cfg_.depth;
        fprintf(stderr, "{\"depth\": {\"row\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"min\": \"%a\", \"max\": \"%a\", \"slices\": %d}}\n",
                d.row[0], d.row[1], d.row[2], d.row[3], d.min, d.max, d.slices);
      }
      if (cfg_.sweep_given) {  // and the sweep: --rotate X,Y:<angles[f]> on the matrix above reproduces frame f
        static const char *const kAxes[4] = {"zr", "zi", "cr", "ci"};
        const cb::Sweep &w = cfg_.sweep;
        fprintf(stderr, "{\"sweep\": {\"axes\": [\"%s\", \"%s\"], \"from\": \"%a\", \"to\": \"%a\", \"frames\": %d, \"angles\": [",
                kAxes[w.axis_x], kAxes[w.axis_y], w.deg0, w.deg1, w.frames);
        for (int f = 0; f < w.frames; ++f) fprintf(stderr, "%s\"%a\"", f ? ", " : "", sweep_angles_[(size_t) f]);
        fprintf(stderr, "]}}\n");
      }
      if (cfg_.depth_palette()) {  // and the colours of its slices
        print_stops("depth_palette", cfg_.depth_palette_stops);
        fprintf(stderr, "}\n");
      }
      if (cfg_.palette()) {  // and the colours
        print_stops("palette", cfg_.palette_stops);
        fprintf(stderr, "}\n");
      }
      fflush(stderr);
    }
    if (cfg_.density.radius > 0 && cfg_.print_stats) {  // on any run: the filter as given and the table made of it
      uint64_t table[CB_DENSITY_MAX_RADIUS + 1];
      if (cb_density_thresholds(cfg_.density.radius, cfg_.density.alpha, cfg_.density.n0, table) != 0) return 1;  // (parsed)
      fprintf(stderr, "{\"density_filter\": {\"radius\": %d, \"alpha\": \"%a\", \"n0\": %llu, \"thresholds\": [",
              cfg_.density.radius, cfg_.density.alpha, (unsigned long long) cfg_.density.n0);
      for (int r = 1; r <= cfg_.density.radius; ++r) fprintf(stderr, "%s%llu", r > 1 ? ", " : "", (unsigned long long) table[r]);
      fprintf(stderr, "]}}\n");
      fflush(stderr);
    }
    if (cfg_.equalize && cfg_.print_stats) {  // likewise
      fprintf(stderr, "{\"equalize\": true}\n");
      fflush(stderr);
    }
    if (cfg_.local_equalize.tx > 0 && cfg_.print_stats) {  // likewise: the grid and the clip in 1/256ths
      fprintf(stderr, "{\"local_equalize\": {\"tiles\": [%d, %d], \"clip_q\": %u}}\n", cfg_.local_equalize.tx,
              cfg_.local_equalize.ty, (unsigned) cfg_.local_equalize.clip_q);
      fflush(stderr);
    }
    setup();
    load_inprogress();
    load_rng_state();
    render();
    save_inprogress();
    save_rng_state();
    if (out_.shape == cb::Shape::kChannels) {
      save_channels();
      if (cfg_.color_file) save_color();
    } else {
      printf("Saving image.\n");
      save_image(cfg_.output_image);
      printf("Done! Output image saved: %s\n", cfg_.output_image);
    }
    release();
    return 0;
  }

 private:
  Settings cfg_;
  cb::Output out_;  // what the flags make of the output: asked for the planes, the image and how it is saved
  cb_renderer *renderer_ = nullptr;      // rank 0: loads, receives the reduced histogram, tone-maps, saves
  // --gpus N: ranks 1..N-1, one per further device, subsequences [r T, (r+1) T) of the
  // same seed; their histograms are summed onto rank 0 once, after the pass loop (cb_renderers_reduce)
  std::vector<cb_renderer *> peers_;
  cb_pixel *counts_ = nullptr;   // host mirror of the histogram (only with -s or --tonemap host)
  uint16_t *gray_ = nullptr;  // the image: of one plane at a time (one gray plane, --channel), else of all the planes
  bool gray_is_big_endian_ = false;
  std::vector<uint16_t> color_grays_;  // --color with --tonemap host: the three planes' values, kept for the compose
  std::vector<cb_pixel> filtered_;  // --density-filter with --tonemap host: the counters the last image was mapped from
  uint64_t host_equalized_[3] = {0, 0, 0};  // --equalize with --tonemap host: lit, keys, levels of the last image
  uint64_t host_local_[3] = {0, 0, 0};  // --local-equalize with --tonemap host: lit, lit tiles, moved of the last image
  std::vector<double> frames_, sweep_angles_;  // --sweep: the F matrices and their angles (cb_frames_from_sweep)

  bool need_host_counts() const { return cfg_.inprogress_file != nullptr || cfg_.host_tonemap; }

  uint64_t pixel_count() const { return (uint64_t) cfg_.canvas.w * (uint64_t) cfg_.canvas.h; }
  uint64_t planes() const { return (uint64_t) out_.planes; }
  // the planes of one image: --channel's and the one gray plane are mapped and saved one at a time
  uint64_t image_planes() const { return kImageOf[(int) out_.sink] ? planes() : 1u; }
  uint64_t buffer_bytes() const { return planes() * pixel_count() * sizeof(cb_pixel); }

  void release() {  // cudabrot.cu:112-119
    for (cb_renderer *p : peers_) cb_renderer_destroy(p);
    peers_.clear();
    cb_renderer_destroy(renderer_);
    renderer_ = nullptr;
    free(gray_);
    gray_ = nullptr;
    free(counts_);
    counts_ = nullptr;
  }

  [[noreturn]] void die() {
    release();
    exit(1);
  }

  // The reference's device-error line (cudabrot.cu:134-141), wording kept: scripts may match on it.
  void check(int rc, const char *what, int line) {
    if (rc == 0) return;
    printf("CUDA error %d (%s) in %s, line %d (%s)\n", rc, cb_error_string(rc), __FILE__, line,
           what);
    die();
  }
#define CB_CHECK(call) check((call), #call, __LINE__)

  // The device table of a list of stops: `entries` colours interpolated between them.
  std::vector<uint32_t> table_of(const cb::Stops &stops, size_t entries) {
    std::vector<uint32_t> lut(entries);
    CB_CHECK(cb_palette_from_stops(stops.at, stops.n, lut.data(), (uint32_t) lut.size()));
    return lut;
  }

  void setup() {  // cudabrot.cu:153-189
    float gpu_mib = (float) (buffer_bytes() + cb_rng_state_bytes(CB_DEFAULT_THREADS));
    gpu_mib /= (1024.0 * 1024.0);
    float cpu_mib = (float) (buffer_bytes() + pixel_count() * sizeof(uint16_t));
    cpu_mib /= (1024.0 * 1024.0);
    printf("Approximate memory needed: %.03f MiB GPU, %.03f MiB CPU\n", gpu_mib, cpu_mib);
    // CUDABROT_AMD_FAKE_GPUS=1: every rank on device -d (rehearsal of --gpus on a one-GPU box)
    const bool fake = cb_debug_knob("CUDABROT_AMD_FAKE_GPUS") != nullptr;
    for (int r = 0; r < cfg_.gpus; ++r) {
      cb_renderer *one = nullptr;
      const int device = cfg_.device + (fake ? 0 : r);
      const uint64_t first = (uint64_t) r * CB_DEFAULT_THREADS;
      if (cfg_.n_channels > 0) {
        CB_CHECK(cb_renderer_create_channels(&one, device, &cfg_.canvas, cfg_.channel_window, cfg_.n_channels,
                                             cfg_.seed, first, CB_DEFAULT_THREADS));
      } else {
        CB_CHECK(cb_renderer_create(&one, device, &cfg_.canvas, &cfg_.iterations, cfg_.seed, first,
                                    CB_DEFAULT_THREADS));
      }
      if (r == 0) {
        renderer_ = one;
      } else {
        peers_.push_back(one);
      }
    }
    if (cfg_.julia) {
      CB_CHECK(cb_renderer_set_julia(renderer_, cfg_.projection, cfg_.julia_c));
    } else if (cfg_.plotted()) {
      CB_CHECK(cb_renderer_set_projection(renderer_, cfg_.projection));
    }
    if (cfg_.depth_palette()) {  // after the plane and c: the table of the stops, one entry per slice
      const std::vector<uint32_t> lut = table_of(cfg_.depth_palette_stops, (size_t) cfg_.depth.slices);
      CB_CHECK(cb_renderer_set_depth_palette(renderer_, &cfg_.depth, lut.data(), (uint32_t) lut.size()));
    } else if (cfg_.depth_given) {
      CB_CHECK(cb_renderer_set_depth(renderer_, &cfg_.depth));  // after the plane and c
    }
    if (cfg_.sweep_given) CB_CHECK(cb_renderer_set_frames(renderer_, frames_.data(), cfg_.sweep.frames));  // likewise
    if (cfg_.phoenix) CB_CHECK(cb_renderer_set_phoenix(renderer_, cfg_.phoenix_p));  // likewise
    if (cfg_.period_palette()) {  // likewise: the table of the stops, one entry per period up to the largest given
      const std::vector<uint32_t> lut = table_of(cfg_.period_stops, (size_t) cfg_.period_entries());
      CB_CHECK(cb_renderer_set_period_palette(renderer_, lut.data(), (uint32_t) lut.size(), cfg_.period_eps));
    } else if (cfg_.bounded) {
      CB_CHECK(cb_renderer_set_bounded(renderer_));  // likewise
    }
    if (cfg_.white_clip > 0.0) CB_CHECK(cb_renderer_set_white_clip(renderer_, cfg_.white_clip));  // an output setting
    if (cfg_.density.radius > 0) {  // likewise
      CB_CHECK(cb_renderer_set_density_filter(renderer_, cfg_.density.radius, cfg_.density.alpha, cfg_.density.n0));
    }
    if (cfg_.equalize) CB_CHECK(cb_renderer_set_equalize(renderer_, 1));  // likewise
    if (cfg_.local_equalize.tx > 0) {  // likewise
      CB_CHECK(cb_renderer_set_local_equalize(renderer_, cfg_.local_equalize.tx, cfg_.local_equalize.ty,
                                              cfg_.local_equalize.clip_q));
    }
    if (cfg_.palette()) {  // after the plane and c: the table of the stops, one entry per escape index below -m
      const std::vector<uint32_t> lut = table_of(cfg_.palette_stops, (size_t) cfg_.iterations.max_escape_iterations);
      CB_CHECK(cb_renderer_set_palette(renderer_, lut.data(), (uint32_t) lut.size()));
    }
    if (need_host_counts()) {
      counts_ = (cb_pixel *) calloc(1, buffer_bytes());
      if (!counts_) die();
    }
    gray_ = (uint16_t *) calloc(image_planes() * pixel_count(), sizeof(uint16_t));
    if (!gray_) {
      printf("Failed allocating grayscale image.\n");
      die();
    }
  }

  void load_inprogress() {  // cudabrot.cu:215-258; the file work is state_files.cpp's
    if (!cfg_.inprogress_file) return;
    const cb::FileResult res = cb::load_state_file(cfg_.inprogress_file, (uint32_t) cfg_.canvas.w, (uint32_t) cfg_.canvas.h,
                                                   (uint32_t) planes(), counts_,
                                                   cfg_.raw_state ? cb::StateFormat::kRaw : cb::StateFormat::kNative);
    if (res == cb::FileResult::kError) die();
    if (res == cb::FileResult::kOk) CB_CHECK(cb_renderer_write_histogram(renderer_, counts_));
  }

  void save_inprogress() {  // cudabrot.cu:262-280
    if (!cfg_.inprogress_file) return;
    if (cb::save_state_file(cfg_.inprogress_file, (uint32_t) cfg_.canvas.w, (uint32_t) cfg_.canvas.h, (uint32_t) planes(),
                            counts_, cfg_.raw_state ? cb::StateFormat::kRaw : cb::StateFormat::kNative) ==
        cb::FileResult::kError) {
      die();
    }
  }

  // True-resume sidecar (extension, off unless --rng-state is given).  The -s buffer
  // is the histogram only, so the reference -- and this program by default -- replays seed 1337 from
  // the start when it resumes (cudabrot.cu:179,215-258).  The sidecar keeps the generator states of every
  // rank, so that buffer + sidecar continue the sample stream: P1 passes, save, resume, P2 passes gives the
  // histogram of one run of P1 + P2 passes -- with --gpus N as well (N generators, the same N to resume).
  uint64_t passes_before_ = 0, passes_this_run_ = 0;

  cb_renderer *rank_renderer(int r) { return r == 0 ? renderer_ : peers_[(size_t) r - 1]; }

  void load_rng_state() {
    if (!cfg_.rng_state_file) return;
    std::vector<std::vector<unsigned char>> blobs;
    const cb::FileResult res =
        cb::load_rng_sidecar(cfg_.rng_state_file, cfg_.seed, CB_DEFAULT_THREADS, (uint32_t) cfg_.gpus,
                             cb_rng_state_bytes(CB_DEFAULT_THREADS), &blobs, &passes_before_);
    if (res == cb::FileResult::kError) die();
    if (res != cb::FileResult::kOk) return;
    for (int r = 0; r < cfg_.gpus; ++r) {
      CB_CHECK(cb_renderer_write_rng_states(rank_renderer(r), blobs[(size_t) r].data()));
    }
  }

  void save_rng_state() {
    if (!cfg_.rng_state_file) return;
    std::vector<std::vector<unsigned char>> blobs((size_t) cfg_.gpus,
                                                  std::vector<unsigned char>(cb_rng_state_bytes(CB_DEFAULT_THREADS)));
    for (int r = 0; r < cfg_.gpus; ++r) {
      CB_CHECK(cb_renderer_read_rng_states(rank_renderer(r), blobs[(size_t) r].data()));
    }
    if (cb::save_rng_sidecar(cfg_.rng_state_file, cfg_.seed, CB_DEFAULT_THREADS, passes_before_ + passes_this_run_,
                             blobs) == cb::FileResult::kError) {
      die();
    }
  }

  // The pass loop (cudabrot.cu:471-501).  Launch length follows the measured pass time so that the
  // clock and the quit flag are looked at about every 0.2 s.
  void render() {
    printf("Calculating Buddhabrot.\n");
    const bool by_clock = cfg_.fixed_passes < 0;
    if (by_clock) {
      if (cfg_.seconds_to_run < 0) {
        printf("Press ctrl+C to finish.\n");
      } else {
        printf("Running for %.03f seconds.\n", cfg_.seconds_to_run);
      }
    }
    fflush(stdout);
    const int variant = cfg_.kernel_variant | (cfg_.burning_ship ? CB_KERNEL_FLAG_BURNING_SHIP : 0) |
                        (cfg_.anti ? CB_KERNEL_FLAG_ANTI : 0) | (cfg_.power ? CB_KERNEL_POWER(cfg_.power) : 0) |
                        (cfg_.formula ? CB_KERNEL_FORMULA(cfg_.formula) : 0);
    if (cfg_.focus.on) set_focus(variant);
    if (cfg_.aim.on) set_aim(variant);
    // what the reference allocates in SetupCUDA, before its clock starts (cudabrot.cu:153-189,476)
    CB_CHECK(cb_renderer_prepare(renderer_, variant));
    for (cb_renderer *p : peers_) CB_CHECK(cb_renderer_prepare(p, variant));
    const double t0 = wall_seconds();
    // The pass loop.  One GPU: batches of `next` reference passes, sized so that the clock and the quit flag are
    // looked at every ~0.2 s.  --gpus N: render_sharded (persistent rank threads and a shared pass budget).
    const double launch_seconds = 0.2;
    long done = 0, next = 1;  // passes per rank
    if (cfg_.gpus > 1) {
      done = render_sharded(variant, by_clock, t0);
    } else {
      while (!g_quit_requested) {
        if (!by_clock) {
          if (done >= cfg_.fixed_passes) break;
          next = cfg_.fixed_passes - done;
          if (next > 256) next = 256;
        }
        CB_CHECK(cb_renderer_render_passes(renderer_, (uint32_t) next, variant));
        done += next;
        if (!by_clock) continue;
        const double elapsed = wall_seconds() - t0;
        if (cfg_.seconds_to_run >= 0 && elapsed > cfg_.seconds_to_run) break;
        double budget = launch_seconds;
        if (cfg_.seconds_to_run >= 0 && cfg_.seconds_to_run - elapsed < budget) {
          budget = cfg_.seconds_to_run - elapsed;
        }
        const double per_pass = elapsed / (double) done;
        next = per_pass > 0 ? (long) (budget / per_pass) : next * 2;
        if (next < 1) next = 1;
        if (next > 4096) next = 4096;
        if (next > 128) next -= next % 128;  // whole launches of 128 passes (cb_renderer's): a short launch drains badly
      }
    }
    passes_this_run_ = (uint64_t) done;  // per rank: what the generators have consumed
    done *= cfg_.gpus;                   // reference-sized passes over all ranks
    if (!peers_.empty()) {  // the one exchange of the path: sum the shards onto rank 0
      std::vector<cb_renderer *> all(1, renderer_);
      all.insert(all.end(), peers_.begin(), peers_.end());
      CB_CHECK(cb_renderers_reduce(all.data(), (int) all.size()));
    }
    if (need_host_counts()) {
      CB_CHECK(cb_renderer_read_histogram(renderer_, counts_));  // cudabrot.cu:496-497
    } else {
      CB_CHECK(cb_renderer_finish(renderer_));
    }
    printf("%ld Buddhabrot passes took %f seconds.\n", done, wall_seconds() - t0);
    if (cfg_.print_stats) print_stats();
    if (out_.shape != cb::Shape::kChannels) make_image(0);  // (--channel: plane by plane, where each is saved)
  }

  // --focus: the probe and the cell list, before the clock of the pass loop starts.  The probe runs on generators of its
  // own, so a run resumed with -s and --rng-state finds the list of the run it continues.
  void set_focus(int variant) {
    set_cells("Focus", cfg_.focus, cb_renderer_set_focus, CB_ERROR_FOCUS_EMPTY, cb_renderer_focus_cells, variant);
  }

  // --aim: likewise for a plotted render, after every setter that makes the renderer what it is.
  void set_aim(int variant) {
    set_cells("Aim", cfg_.aim, cb_renderer_set_aim, CB_ERROR_AIM_EMPTY, cb_renderer_aim_cells, variant);
  }

  // Set, report an empty list, print the sampling line: `set` and `cells` are the render's setter and its cell count,
  // `empty` the setter's code for a probe that marked nothing, `name` what the lines call the render.
  void set_cells(const char *name, const cb::CellFlags &f, int (*set)(cb_renderer *, int, uint32_t, int, int), int empty,
                 int (*cells)(const cb_renderer *, uint32_t *, uint32_t *), int variant) {
    const int rc = set(renderer_, f.level, (uint32_t) f.probe, f.dilate, variant);
    if (rc == empty) {
      printf("%s: no sample of the %ld probe passes reaches the canvas; nothing to render.\n", name, f.probe);
      die();
    }
    CB_CHECK(rc);
    uint32_t n_cells = 0, n_total = 0;
    CB_CHECK(cells(renderer_, &n_cells, &n_total));
    printf("%s: sampling %u of %u cells of side 2^-%d (%ld probe passes, dilated by %d).\n", name, n_cells, n_total,
           f.level, f.probe, f.dilate);
    fflush(stdout);
  }

  // The pass loop of --gpus N.  One persistent host thread per rank; the ranks do not meet at batch
  // ends (boxes differ by 3-4 %, and every rendezvous would cost the faster ranks that much plus a restart of their
  // pipelines).  What they share is a pass BUDGET: `granted`, raised by the main thread alone -- which alone reads
  // the clock and the quit flag -- about 0.4 s ahead of the slowest rank; a rank renders whatever the budget allows
  // beyond its own count, in whole launches.  When the run ends (--passes reached, -t over, Ctrl+C) the budget is
  // frozen at what the furthest rank has been given and every rank completes it: an N-GPU run is "N T threads for
  // P passes" however it ends, which is what makes it reproducible and resumable (--rng-state).  A device error on
  // any rank stops the budget; it is reported from the main thread after every worker has been joined.
  long render_sharded(int variant, bool by_clock, double t0) {
    const int n = cfg_.gpus;
    struct Shared {
      std::mutex m;
      std::condition_variable cv;
      long granted = 0;
      bool closed = false;            // the budget is final
      std::vector<long> done, taken;  // per rank: passes rendered / rendered + in flight
      std::vector<int> rc;
    } sh;
    sh.done.assign((size_t) n, 0);
    sh.taken.assign((size_t) n, 0);
    sh.rc.assign((size_t) n, 0);
    std::vector<std::thread> workers;
    for (int k = 0; k < n; ++k) {
      workers.emplace_back([&, k] {
        cb_renderer *mine = rank_renderer(k);
        for (;;) {
          long piece = 0;
          {
            std::unique_lock<std::mutex> lock(sh.m);
            sh.cv.wait(lock, [&] { return sh.granted > sh.done[(size_t) k] || sh.closed; });
            piece = sh.granted - sh.done[(size_t) k];
            if (piece <= 0) return;       // closed and complete
            if (piece > 1024) piece = 1024;  // (a call returns when its launches are done: look at the budget again)
            sh.taken[(size_t) k] = sh.done[(size_t) k] + piece;
          }
          const int rc = cb_renderer_render_passes(mine, (uint32_t) piece, variant);
          std::lock_guard<std::mutex> lock(sh.m);
          if (rc != 0) {
            sh.rc[(size_t) k] = rc;
            sh.taken[(size_t) k] = sh.done[(size_t) k];
            sh.closed = true;             // no further grants; the others finish what they have taken
            sh.granted = 0;
            for (int j = 0; j < n; ++j) sh.granted = sh.taken[(size_t) j] > sh.granted ? sh.taken[(size_t) j] : sh.granted;
            sh.cv.notify_all();
            return;
          }
          sh.done[(size_t) k] += piece;
          sh.cv.notify_all();
        }
      });
    }
    {
      std::unique_lock<std::mutex> lock(sh.m);
      const long lead_min = 128;  // whole launches of cb_renderer (a short launch drains badly)
      if (!by_clock) {
        sh.granted = cfg_.fixed_passes > 0 ? cfg_.fixed_passes : 0;
        if (sh.granted == 0) sh.closed = true;
      } else {
        sh.granted = 1;  // the first pass calibrates the pace
      }
      sh.cv.notify_all();
      for (;;) {
        bool failed = false;
        long slowest = sh.granted, furthest = 0;
        for (int k = 0; k < n; ++k) {
          failed = failed || sh.rc[(size_t) k] != 0;
          slowest = sh.done[(size_t) k] < slowest ? sh.done[(size_t) k] : slowest;
          furthest = sh.taken[(size_t) k] > furthest ? sh.taken[(size_t) k] : furthest;
        }
        if (failed || sh.closed) break;
        const double elapsed = wall_seconds() - t0;
        const bool time_up = by_clock && cfg_.seconds_to_run >= 0 && elapsed > cfg_.seconds_to_run && slowest >= 1;
        const bool all_done = !by_clock && slowest >= sh.granted;
        if (g_quit_requested || time_up || all_done) {
          // final budget: what the furthest rank has been given (at least one pass, like the reference's loop)
          sh.granted = furthest > 1 ? furthest : 1;
          if (!by_clock && !g_quit_requested) sh.granted = cfg_.fixed_passes;
          sh.closed = true;
          sh.cv.notify_all();
          break;
        }
        if (by_clock && slowest >= 1) {
          const double per_pass = elapsed / (double) slowest;  // the slowest rank's pace
          // whole launches of cb_renderer, to the end: the clock acts at the granularity of a batch, as it does on one GPU
          // (a budget that shrank with the time left made the ranks issue 1-pass launches, which drain badly)
          const double ahead = 2.0 * launch_seconds_;
          long lead = per_pass > 0 ? (long) (ahead / per_pass) : lead_min;
          if (lead > 4096) lead = 4096;
          lead -= lead % lead_min;
          if (lead < lead_min) lead = lead_min;
          if (slowest + lead > sh.granted) {
            sh.granted = slowest + lead;
            sh.cv.notify_all();
          }
        }
        sh.cv.wait_for(lock, std::chrono::milliseconds(10));
      }
      // every rank completes the final budget
      sh.cv.wait(lock, [&] {
        for (int k = 0; k < n; ++k) {
          if (sh.rc[(size_t) k] == 0 && sh.done[(size_t) k] < sh.granted) return false;
        }
        return true;
      });
    }
    for (std::thread &w : workers) w.join();
    for (int r = 0; r < n; ++r) {
      if (sh.rc[(size_t) r] != 0) printf("GPU %d of %d:\n", r, n);
      CB_CHECK(sh.rc[(size_t) r]);
    }
    return sh.granted;
  }
  static constexpr double launch_seconds_ = 0.2;

  // The reference's host loop over `rows` rows of the counters at `hist` -- with --white-clip, the clipped one; with
  // --equalize, the equalised one, whose bins and table are made once here and what they found kept (host_equalized_), as a
  // renderer keeps it; with --local-equalize, the locally equalised one over the planes of the canvas's height, what it
  // found kept likewise (host_local_); with --density-filter, over the filtered counters (filtered_): planes of the
  // canvas's height, smoothed in groups of `group`.
  void host_tone_map(const cb_pixel *hist, int rows, int group, uint16_t *gray, uint64_t *max, double *scale) {
    if (cfg_.density.radius > 0) {
      uint64_t table[CB_DENSITY_MAX_RADIUS + 1];
      CB_CHECK(cb_density_thresholds(cfg_.density.radius, cfg_.density.alpha, cfg_.density.n0, table));
      filtered_.resize((size_t) rows * (size_t) cfg_.canvas.w);
      CB_CHECK(cb_density_filter(hist, cfg_.canvas.w, cfg_.canvas.h, rows / cfg_.canvas.h, group, cfg_.density.radius,
                                 table, filtered_.data()));
      hist = filtered_.data();
    }
    if (cfg_.equalize) {  // cb_set_grayscale_pixels_equalized, its steps apart: it does not hand on the table's two numbers
      const uint64_t n = (uint64_t) cfg_.canvas.w * (uint64_t) rows;
      std::vector<uint64_t> bins(CB_EQUALIZE_KEYS);
      std::vector<uint16_t> table(CB_EQUALIZE_KEYS);
      CB_CHECK(cb_equalize_bins(hist, n, bins.data(), &host_equalized_[0], max));
      CB_CHECK(cb_equalize_table(bins.data(), cfg_.gamma_correction, table.data(), &host_equalized_[1], &host_equalized_[2]));
      *scale = ((double) 0xffff) / ((double) *max);
      for (uint64_t i = 0; i < n; ++i) gray[i] = table[cb_equalize_key(hist[i])];
    } else if (cfg_.local_equalize.tx > 0) {
      CB_CHECK(cb_set_grayscale_pixels_local_equalized(hist, cfg_.canvas.w, cfg_.canvas.h, rows / cfg_.canvas.h,
                                                       cfg_.local_equalize.tx, cfg_.local_equalize.ty,
                                                       cfg_.local_equalize.clip_q, cfg_.gamma_correction, gray, max, scale,
                                                       &host_local_[0], &host_local_[1], &host_local_[2]));
    } else if (cfg_.white_clip > 0.0) {
      CB_CHECK(cb_set_grayscale_pixels_white(hist, cfg_.canvas.w, rows, cfg_.gamma_correction, cfg_.white_clip, gray, max,
                                             scale, nullptr));
    } else {
      cb_set_grayscale_pixels(hist, cfg_.canvas.w, rows, cfg_.gamma_correction, gray, max, scale);
    }
  }

  // The "Max value" line (cudabrot.cu:437) of an image over `rows` rows of the counters at `hist` (the host's mirror, read
  // with --tonemap host only) -- and with --white-clip the line of what the clip found: by the host's definition or, on the
  // device path, as the renderer's image call reported it; with --equalize, likewise, the line of what the equalisation
  // found.  With --density-filter both lines speak of the filtered counters, and a line between them says so.
  void print_exposure(uint64_t max, double scale, const cb_pixel *hist, int rows) {
    printf("Max value: %lu, scale: %f\n", (unsigned long) max, scale);
    if (cfg_.density.radius > 0) {
      printf("Density filter: radius %d, alpha %g, n0 %lu (the values above carry 8 fraction bits)\n", cfg_.density.radius,
             cfg_.density.alpha, (unsigned long) cfg_.density.n0);
      if (cfg_.host_tonemap) hist = filtered_.data();  // what host_tone_map mapped
    }
    if (cfg_.equalize) {  // what the equalisation found, by the host's definition or as the renderer's image call reported it
      uint64_t lit = host_equalized_[0], keys = host_equalized_[1], levels = host_equalized_[2];
      if (!cfg_.host_tonemap) CB_CHECK(cb_renderer_last_equalize(renderer_, &lit, &keys, &levels));
      printf("Equalized: %lu lit pixels in %lu keys, %lu output levels\n", (unsigned long) lit, (unsigned long) keys,
             (unsigned long) levels);
    }
    if (cfg_.local_equalize.tx > 0) {  // likewise
      uint64_t lit = host_local_[0], lit_tiles = host_local_[1], moved = host_local_[2];
      if (!cfg_.host_tonemap) CB_CHECK(cb_renderer_last_local_equalize(renderer_, &lit, &lit_tiles, &moved));
      printf("Locally equalized: %dx%d tiles, clip %u/256, %lu lit pixels in %lu lit tiles, %lu counts moved\n",
             cfg_.local_equalize.tx, cfg_.local_equalize.ty, (unsigned) cfg_.local_equalize.clip_q, (unsigned long) lit,
             (unsigned long) lit_tiles, (unsigned long) moved);
    }
    if (!(cfg_.white_clip > 0.0)) return;
    uint64_t white = 0, lit = 0, clipped = 0;
    if (cfg_.host_tonemap) {
      CB_CHECK(cb_white_count(hist, (uint64_t) cfg_.canvas.w * (uint64_t) rows, cfg_.white_clip, &white, &lit, &clipped));
    } else {
      CB_CHECK(cb_renderer_last_white(renderer_, &white, &lit, &clipped));
    }
    printf("White value: %lu (%g%% of %lu lit pixels may clip, %lu do)\n", (unsigned long) white, cfg_.white_clip,
           (unsigned long) lit, (unsigned long) clipped);
  }

  // The image of the run into gray_: of `plane` alone where the sink has an image per plane, else of all its planes at once,
  // as one w x N*h image against their common maximum -- on the device (only the 16-bit image crosses to the host), or with
  // --tonemap host by the reference's host loop over the same rows; what is saved is the same bytes.  The loop's values are
  // the host's: one plane keeps them for cb_save_image (and for --color's compose); the planes of a stack are swapped into
  // the big-endian values the device hands over; the three planes of a colour image are interleaved into the PPM body first.
  void make_image(int plane) {
    uint64_t max = 0;
    double scale = 0.0;
    const ImageCall image = kImageOf[(int) out_.sink];
    const bool color = out_.shape == cb::Shape::kColor;
    const uint64_t values = image_planes() * pixel_count();
    const int rows = (int) image_planes() * cfg_.canvas.h;
    const cb_pixel *hist = counts_ ? counts_ + (uint64_t) plane * pixel_count() : nullptr;
    if (cfg_.host_tonemap) {
      host_tone_map(hist, rows, color ? 3 : 1, gray_, &max, &scale);
      if (color) {
        const std::vector<uint16_t> planar(gray_, gray_ + values);
        for (uint64_t i = 0; i < pixel_count(); ++i) {
          for (uint64_t j = 0; j < 3; ++j) gray_[3 * i + j] = planar[j * pixel_count() + i];
        }
      }
      if (image) {  // all planes make one image: the device's byte order
        for (uint64_t i = 0; i < values; ++i) gray_[i] = (uint16_t) ((gray_[i] << 8) | (gray_[i] >> 8));
      }
    } else if (image) {
      CB_CHECK(image(renderer_, cfg_.gamma_correction, cfg_.tone_mode, gray_, &max, &scale));
    } else {
      CB_CHECK(cb_renderer_grayscale_plane(renderer_, plane, cfg_.gamma_correction, cfg_.tone_mode, gray_, &max, &scale));
    }
    gray_is_big_endian_ = image || !cfg_.host_tonemap;
    print_exposure(max, scale, hist, rows);
  }

  // --depth, --sweep: N binary PGMs back to back in one file (Netpbm's format allows a sequence of images), each
  // SaveImage's (cudabrot.cu:548-577); 0, or 1/2/3 = open / header / pixel-data failure as cb_save_image.
  int save_plane_images(const char *path) {
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    int rc = 0;
    for (uint64_t s = 0; s < planes() && rc == 0; ++s) {
      if (fprintf(f, "P5\n%d %d\n65535\n", cfg_.canvas.w, cfg_.canvas.h) <= 0) {
        rc = 2;
      } else if (fwrite(gray_ + s * pixel_count(), sizeof(uint16_t), pixel_count(), f) != pixel_count()) {
        rc = 3;
      }
    }
    if (fclose(f) != 0 && rc == 0) rc = 3;
    return rc;
  }

  // Fused multi-channel render: one image per window.
  void save_channels() {
    for (int j = 0; j < cfg_.n_channels; ++j) {
      printf("Channel %d: %d max iterations, %d min iterations.\n", j,
             cfg_.channel_window[j].max_escape_iterations, cfg_.channel_window[j].min_escape_iterations);
      make_image(j);
      if (cfg_.color_file && cfg_.host_tonemap) {  // before save_image swaps gray_ in place
        color_grays_.resize(3 * pixel_count());
        memcpy(color_grays_.data() + (uint64_t) j * pixel_count(), gray_, pixel_count() * sizeof(uint16_t));
      }
      printf("Saving image.\n");
      save_image(cfg_.channel_file[j].c_str());
      printf("Done! Output image saved: %s\n", cfg_.channel_file[j].c_str());
    }
  }

  // --color: the three planes composed into one RGB image, on the device (only the image crosses to the host) or, with
  // --tonemap host, by the host restatement from the planes' values; the bytes are the same.  With --gpus N this
  // is rank 0's histogram, after the reduce.
  void save_color() {
    std::vector<uint16_t> rgb_be(3 * pixel_count());
    uint16_t levels[6] = {0, 0, 0, 0, 0, 0};
    if (cfg_.host_tonemap) {
      const uint16_t *planes[3] = {color_grays_.data(), color_grays_.data() + pixel_count(),
                                   color_grays_.data() + 2 * pixel_count()};
      CB_CHECK(cb_compose_color(planes, cfg_.canvas.w, cfg_.canvas.h, &cfg_.color, rgb_be.data(), levels));
    } else {
      const int planes[3] = {0, 1, 2};
      CB_CHECK(cb_renderer_color_image(renderer_, planes, cfg_.gamma_correction, cfg_.tone_mode, &cfg_.color,
                                       rgb_be.data(), levels));
    }
    printf("Color levels: black %u %u %u, white %u %u %u\n", levels[0], levels[2], levels[4], levels[1], levels[3],
           levels[5]);
    printf("Saving color image.\n");
    report_save(cb_save_ppm_be(cfg_.color_file, rgb_be.data(), cfg_.canvas.w, cfg_.canvas.h));
    printf("Done! Color image saved: %s\n", cfg_.color_file);
  }

  // The cells / total / fraction piece of the stats line of a focused ("focus") or an aimed ("aim") run.
  void print_cells(const char *key, int (*cells)(const cb_renderer *, uint32_t *, uint32_t *)) {
    uint32_t n_cells = 0, n_total = 0;
    CB_CHECK(cells(renderer_, &n_cells, &n_total));
    fprintf(stderr, "\"%s_cells\": %u, \"%s_total\": %u, \"%s_fraction\": %.9g, ", key, n_cells, key, n_total, key,
            n_total ? (double) n_cells / (double) n_total : 0.0);
  }

  void print_stats() {
    cb_counters c;
    CB_CHECK(cb_renderer_read_counters(renderer_, &c));
    for (cb_renderer *p : peers_) {  // workload counters add up over the ranks (the clocks are rank 0's)
      cb_counters o;
      CB_CHECK(cb_renderer_read_counters(p, &o));
      c.samples += o.samples;
      c.rejected += o.rejected;
      c.never_escaped += o.never_escaped;
      c.too_fast += o.too_fast;
      c.recorded += o.recorded;
      c.iterate_steps += o.iterate_steps;
      c.replay_steps += o.replay_steps;
      c.increments += o.increments;
      c.skipped_steps += o.skipped_steps;
      c.status |= o.status;
    }
    // the level of the interior map every rank's last launch used (0: none), rank by rank
    std::string levels = std::to_string(cb_renderer_interior_map_level(renderer_));
    for (cb_renderer *p : peers_) levels += ", " + std::to_string(cb_renderer_interior_map_level(p));
    fprintf(stderr, "{\"interior_map_levels\": [%s], ", levels.c_str());
    // the part of the plane the samples come from: the factor between focused (aimed) and uniform sample counts
    if (cfg_.focus.on) print_cells("focus", cb_renderer_focus_cells);
    if (cfg_.aim.on) print_cells("aim", cb_renderer_aim_cells);
    fprintf(stderr,
            "\"samples\": %llu, \"rejected\": %llu, \"never_escaped\": %llu, \"too_fast\": %llu, "
            "\"recorded\": %llu, \"iterate_steps\": %llu, \"replay_steps\": %llu, "
            "\"increments\": %llu, \"skipped_steps\": %llu, \"status\": %llu, \"cycles_head\": %llu, "
            "\"cycles_long\": %llu, "
            "\"cycles_replay\": %llu, \"cycles_total\": %llu, \"rt_span\": %llu, \"rt_wave_life_sum\": %llu}\n",
            (unsigned long long) c.samples, (unsigned long long) c.rejected,
            (unsigned long long) c.never_escaped, (unsigned long long) c.too_fast,
            (unsigned long long) c.recorded, (unsigned long long) c.iterate_steps,
            (unsigned long long) c.replay_steps, (unsigned long long) c.increments,
            (unsigned long long) c.skipped_steps,
            (unsigned long long) c.status, (unsigned long long) c.cycles_head,
            (unsigned long long) c.cycles_long, (unsigned long long) c.cycles_replay,
            (unsigned long long) c.cycles_total,
            (unsigned long long) (c.rt_last_end ? c.rt_last_end - ~c.rt_not_first_start : 0),
            (unsigned long long) c.rt_wave_life_sum);
  }

  // The image make_image left, as the file of its shape (cudabrot.cu:548-577: failures are reported and the run still ends
  // with 0).
  void save_image(const char *path) {
    const int w = cfg_.canvas.w, h = cfg_.canvas.h;
    report_save(out_.shape == cb::Shape::kColor   ? cb_save_ppm_be(path, gray_, w, h)
                : out_.shape == cb::Shape::kStack ? save_plane_images(path)
                : gray_is_big_endian_             ? cb_save_image_be(path, gray_, w, h)
                                                  : cb_save_image(path, gray_, w, h));
  }

  static void report_save(int rc) {
    static const char *const kWhy[] = {nullptr, "Failed opening output image.", "Failed writing pgm header.",
                                       "Failed writing pixel data."};
    if (rc >= 1 && rc <= 3) printf("%s\n", kWhy[rc]);
  }
#undef CB_CHECK
};

}  // namespace

// cudabrot.cu:756-760
extern "C" void on_sigint(int signal_number) {
  g_quit_requested = 1;
  printf("Signal %d received, waiting for current pass to finish...\n", signal_number);
}

int main(int argc, char **argv) {
  const Settings settings = cb::parse_arguments(argc, argv);
  if (signal(SIGINT, on_sigint) == SIG_ERR) {  // cudabrot.cu:774-778
    printf("Failed setting signal handler.\n");
    return 1;
  }
  Run run(settings);
  return run.execute();
}
