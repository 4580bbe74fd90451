// kernels.h -- internal launch interface between the C ABI (capi.hip) and the device code.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cudabrot_amd.h"

namespace cb {

// Number of GF(2) jump matrices kept on the device: A^(2^(67+b)), b in [0,64).
constexpr int kSeqJumpMatrices = 64;
constexpr int kMatrixWords = 160 * 5;

// Host: fills out[kSeqJumpMatrices][kMatrixWords] (xorwow_host.cpp).
void build_sequence_jump_matrices(uint32_t *out);
// Host: seeded XORWOW state before any jump (rocrand_xorwow.h:104-123): x[0..4], d.
void seed_state(uint64_t seed, uint32_t x[5], uint32_t *d);

// ---- deferred, tile-binned scatter (scatter.hip) ------------------------------------------------
//
// Random u64 atomics run at ~24 G/s on MI355X whatever the schedule (one 64-byte memory-side request
// each), which caps every configuration of this path.  With a workspace, the REPLAY stage therefore
// does not touch the histogram: each wave appends the visited pixels as packed (row << 16 | col)
// words to its own region of a stream in HBM (coalesced stores).  After the draw kernel the stream is
// cut into REGIONS of 32768 entries; every region is sorted by 128x128-pixel tile on its own, inside one
// workgroup's LDS (no counting pass over the stream, no global prefix sums: the only thing a region
// publishes is where each tile's run starts inside it), and one workgroup per (tile, slice of regions)
// then gathers that tile's runs from the regions, accumulates them in an LDS histogram and adds the tile
// to the u64 histogram with coalesced atomics: one 64-byte request per 8 pixels per slice instead of one
// per increment.
constexpr int kTileShift = 7;
constexpr int kTileSize = 1 << kTileShift;          // 128 x 128 pixels
constexpr int kTilePixels = kTileSize * kTileSize;  // 16384 u32 counters = 64 KiB of LDS
constexpr uint32_t kGroupTiles = 1024;              // keys of one region sort; more tiles: two levels
constexpr uint32_t kMinRegionEntries = 4096;        // below this per wave the workspace is not used
constexpr uint32_t kGroupReplicas = 4;              // level-A keys per group of the two-level sort (scatter.hip)
// Two levels, CHUNKED (up to kChunkedGroupsMax groups of 1024 tiles): level A happens where the words are born.
// A wave's segment of the stream is cut into chunks of kChunkWords words; REPLAY appends a word to the current
// chunk of its GROUP (cursor and limit of every group in the wave's LDS; a full chunk is followed by the next
// free one of the segment) and notes the group of every chunk it opens in chunk_desc.  The scatter then sorts
// REGIONS OF kRegionChunks CHUNKS of one group (lists of chunks instead of stretches of a grouped copy of the
// stream): the stream is written once and read once, where the counting sort of level A read it twice more and
// wrote it once more.
constexpr uint32_t kChunkWords = 1024;
constexpr uint32_t kRegionChunks = 32;              // 32 * 1024 = the 32768 entries of a region sort
constexpr uint32_t kChunkedGroupsMax = 64;          // cursors: 64 x {next word, end of chunk} = 512 B of LDS per wave
// One level, BLOCKED (draw_wide_kernel's stream): a segment is a row of blocks of four slots, 16 bytes on a 16-byte
// boundary; a block holds up to four consecutive points of ONE lane's orbit, and a slot without a point holds
// kStreamSentinel (row and col 65535: a pixel no canvas of at most 1024 tiles has).  Every block the draw kernel writes
// holds a point; a reader takes any.  wave_count[w] counts SLOTS and carries kStreamBlocked; a segment without the
// bit (draw_wave_kernel's, a planted one) is a row of words.  Counts stay below 2^31: a workspace holds fewer
// than 2^32 entries in all (make_bin_layout), and a segment is at most half of it.
constexpr uint32_t kStreamBlocked = 1u << 31;       // in wave_count[w], and in region_count[r] until the region is sorted
constexpr uint32_t kStreamSentinel = 0xffffffffu;

struct BinLayout {
  uint32_t enabled;     // 0: REPLAY adds to the histogram directly
  uint32_t n_waves;     // segments of the stream (= waves of the draw kernel)
  uint32_t cap;         // entries per wave segment (multiple of 8)
  uint32_t n_tiles;     // n_planes * tiles_x * tiles_y
  uint32_t tiles_x;
  uint32_t slice_regions;  // regions one accumulate workgroup gathers from
  // more than kGroupTiles tiles: the stream is first partitioned into groups of 1024 consecutive tiles
  // (level A: count -> scan -> scatter of whole words into `grouped`), and the regions are cut from each
  // group's stretch of `grouped`, so that a region holds tiles of one group only; scatter.hip
  uint32_t two_level;
  uint32_t n_groups;    // 1 with one level
  // two levels and n_groups <= kChunkedGroupsMax: the stream is chunked by group as it is written (above);
  // wave_count then holds the chunks a wave has opened, a_count / a_base count and place CHUNKS, and `grouped`
  // does not exist
  uint32_t chunked;
  uint32_t chunks_per_wave;  // cap / kChunkWords
  uint32_t max_regions;   // size of the region table and row length of run_start
  // Layout of a stream word: col in the low bits, row above it (e_row_shift), and -- fused multi-channel
  // renders only -- the index of the channel (plane) the point goes to above both (e_chan_shift,
  // e_chan_mask; 0 / 0 with one plane).  One channel: row << 16 | col.  The planes are sorted as ONE
  // canvas of n_planes * tiles_y tile rows: tile index = (plane * tiles_y + tile row) * tiles_x + tile
  // column, n_tiles = n_planes * tiles_x * tiles_y, so one sort -> accumulate serves all planes.
  uint32_t e_row_shift, e_col_mask, e_row_mask, e_chan_shift, e_chan_mask;
  uint32_t n_planes, tiles_y;
  unsigned long long plane_pixels;  // w * h: distance between the planes of the histogram
  uint32_t *wave_count;           // [n_waves]            entries written by each wave (| kStreamBlocked: slots, in blocks)
  uint32_t *stream;               // [n_waves][cap]       packed row << 16 | col; blocked: or kStreamSentinel
  uint32_t *a_count;              // [n_groups*replicas][n_waves]  level A counts, then prefix over waves
  unsigned long long *a_base;     // [n_groups*replicas + 1]  level A exclusive prefix over keys
  uint32_t *grouped;              // [n_waves * cap]      the stream, grouped (two levels)
  unsigned long long *region_start;  // [max_regions]     regions of the (grouped) stream: first entry ...
  uint32_t *region_count;         // [max_regions]        ... entries (<= 32768; once sorted: the entries PLACED) ...
  uint32_t *region_group;         // [max_regions]        ... and group (0 with one level)
  uint32_t *owner_first;          // [max(n_waves, groups) + 1]  first region of every wave (one level) / group
  uint32_t *group_first;          // [n_groups]           a group's regions are consecutive: the first ...
  uint32_t *group_regions;        // [n_groups]           ... and how many
  uint32_t *n_regions;            // [1] (+ the slice size and the entries of the launch behind it)
  uint32_t *chunk_desc;           // [n_waves][chunks_per_wave]  chunked: group << 16 | words in the chunk
  uint2 *chunk_list;              // [n_waves * chunks_per_wave]  chunked: {first word, words} of every chunk, by group
  uint16_t *run_start;            // [min(n_tiles, 1024)][max_regions]  where tile k0 + i's run starts in a region
  uint32_t *slice_base;           // [n_tiles + 1]        exclusive prefix of accumulate workgroups per tile
  uint16_t *sorted;               // [n_waves * cap]      in-tile offsets, every region sorted by tile in place
};

// Bytes of a workspace for launches that write about entries_per_wave stream entries per wave (0 if
// the canvas cannot use one: a side above 65536 or more than 262144 tiles over all planes).
size_t bin_workspace_bytes(int w, int h, uint32_t n_waves, double entries_per_wave, int n_planes = 1);
// Bytes of every array of a BinLayout as make_bin_layout carved it (0: the layout has no such array): what
// cb_debug_scatter_layout reports.  The kernels never see it.
struct BinLayoutBytes {
  size_t wave_count, stream, a_count, a_base, grouped, region_start, region_count, region_group, owner_first,
      group_first, group_regions, n_regions, chunk_desc, chunk_list, run_start, slice_base, sorted;
};
// Carves `bytes` at `workspace` into a BinLayout (enabled = 0 if it is too small or the canvas does
// not qualify).  Host arithmetic only: the workspace is not touched.  carved (may be null): the arrays' sizes.
BinLayout make_bin_layout(void *workspace, size_t bytes, int w, int h, uint32_t n_waves, int n_channels = 0,
                          BinLayoutBytes *carved = nullptr);
// region sort -> gather + accumulate on `stream`, after the draw kernel that filled the stream.
hipError_t launch_binned_scatter(const BinLayout &b, unsigned long long *hist, int w, int h,
                                 hipStream_t stream);

struct DrawArgs {
  // canvas (cudabrot.cu:46-58) + exact-reciprocal fast path
  double min_real, min_imag, delta_real, delta_imag, inv_delta_real, inv_delta_imag;
  int w, h, pow2_real, pow2_imag;
  // RN(1 / delta) for any delta: the replay burst's quotient estimate (draw_wave.hip, CB_REPLAY_BIN_DIV)
  double rcp_delta_real, rcp_delta_imag;
  // The replay burst's wave-constant operands, made on the host (capi.hip, make_args) so that the kernel reads
  // them from its argument segment with scalar loads where they are used: neither vector instructions to
  // derive them nor scalar registers to hold them across the other stages.
  //   2 min (the tests R >= 2 min_re on doubled coordinates);
  //   dyadic pixels: scale = 0.5 / delta, offset = -(min / delta)  (pixel = fma(R, scale, offset));
  //   else:          scale = delta, offset = min                  (pixel = (R / 2 - offset) / scale)
  double replay_min2_real, replay_min2_imag;
  double replay_scale_real, replay_scale_imag, replay_offset_real, replay_offset_imag;
  double replay_bound_w, replay_bound_h;  // (double) w, (double) h (draw_wide.hip)
  // Likewise the LONG stage's constants (from max_iter, min_iter and the stage split): iterations left to
  // the stage, the length of an orbit's last, shorter chunk and the l_rem that marks it (~0: none), and the
  // largest l_rem at which an escape is accepted (max_iter - min_iter)
  uint32_t long_steps, tail_steps, tail_value;
  int accept_rem;
  int fast_mid;  // the usual split: MID ends at or before min_iter and the LONG stage follows
  // The LONG stage's chunks test for escape on every tenth step only (draw_wave.hip, iterate_chunk2_sparse):
  // allowed when every escape inside a full LONG chunk is accepted, i.e. min_iter <= long_start.  long_start:
  // first iteration of the LONG stage; tail_start: first iteration of an orbit's last, shorter chunk (which
  // tests every step).
  int sparse_long, long_start, tail_start;
  // what |Z|^2 is compared with at a sparse test step: 16 - 2^-10 (draw_wave.hip, kSparseThreshold).  Any value
  // up to that gives the same result -- a lower one only sends more lanes through the exact decision
  // (CUDABROT_AMD_SPARSE_THRESHOLD: how the tests drive that path, which otherwise runs once in 3e8 test steps)
  double sparse_threshold;
  // iteration control (cudabrot.cu:62-67)
  int max_iter, min_iter;
  // stage split of draw_wave_kernel (plan_stages): HEAD runs iterations [0, head_steps), MID the
  // next mid_steps, LONG the rest
  int head_steps, mid_steps;
  uint32_t n_threads;
  uint32_t samples_per_thread;
  unsigned long long *hist;
  uint32_t *states;  // six planes of n_threads
  cb_counters *counters;
  BinLayout bin;
  // timed variant only, may be null: 8 words per wave {HW_ID, XCC_ID, start, end (100 MHz clock),
  // cycles in HEAD, LONG, REPLAY, total}
  unsigned long long *wave_dump;
  // 1: retire orbits found exactly periodic (default); 0: iterate every sample to max_iter like the
  // reference does (CB_KERNEL_FULL_ITERATE, for measuring the iterate loop against its roofline)
  int check_periodic;
  // Carry-over of in-flight work (may be null).  Draining a launch is expensive: the deepest orbits
  // take hundreds of chunks with almost every lane idle.  With a carry buffer a launch stops when
  // its samples are drawn and leaves queues and orbit slots in the buffer for the next launch; a
  // launch with drain != 0 (and normally no samples) finishes everything.  kCarryWordsPerWave u64
  // words per wave, zeroed by the caller before the first launch.
  unsigned long long *carry;
  int drain;
  // the reference's RENDER_BURNING_SHIP variant (cudabrot.cu:15-17); read by draw_simple_kernel, the
  // wave kernel has a build of its own for it (launch_draw_wave_ship)
  int burning_ship;
  // CB_KERNEL_FLAG_ANTI: the anti-Buddhabrot (the orbits that never escape, draw_anti.hip); read by the capi's
  // dispatch only, the anti kernels are the only ones launched with it set
  int anti;
  // Fused multi-channel render: n_channels > 0 windows [chan_min[j], chan_max[j]) of
  // the escape index; max_iter / min_iter above are then the largest max and the smallest min, and an
  // orbit is replayed once into every channel whose window holds its escape index.  hist is
  // n_channels planes of plane_pixels counters.
  int n_channels;
  int chan_min[CB_MAX_CHANNELS], chan_max[CB_MAX_CHANNELS];
  unsigned long long plane_pixels;
  // The interior map (tools/interior_map.c; null: none): one bit per cell of side 2^-level of the c-plane, re in
  // [-2, 0.5), |im| in [0, 1.25), set where EVERY sample of the cell provably never escapes under the reference's
  // iteration.  draw_wide_kernel's MID stage looks a survivor of HEAD up and retires a marked one as never-escaping
  // instead of iterating it until its orbit repeats.  interior_shift = level - 1 (the kernel's coordinates are doubled).
  const unsigned char *interior_map;
  uint32_t interior_shift, interior_cols, interior_rows;
};

constexpr uint32_t kCarryHeaderWords = 8;
constexpr uint32_t kCarryQueueWords = (2 * 128 + 4 * 96 + 2 * 192 + 192 / 2);  // = sizeof(WaveQueues) / 8
constexpr uint32_t kCarryLanePlanes = 19;
constexpr uint32_t kCarryWordsPerWave = kCarryHeaderWords + kCarryQueueWords + kCarryLanePlanes * 64;
// Behind the per-wave records of a carry buffer: the progress board of the draw kernel's waves, 16 words
// per SIMD (one per wave slot), indexed by (XCC, SE, SH, CU, SIMD).  The waves that share a SIMD post how
// many samples they still have to draw and take their issue priority from their rank (draw_wave.hip).
constexpr uint32_t kSchedKeys = 1u << 16;
constexpr uint32_t kSchedWords = kSchedKeys * 16u;  // u32 words

constexpr uint32_t kDrawBlockThreads = 256;  // 4 waves per workgroup
inline uint32_t draw_wave_count(uint32_t n_threads) {
  return ((n_threads + kDrawBlockThreads - 1u) / kDrawBlockThreads) * (kDrawBlockThreads / 64u);
}

hipError_t launch_rng_init(uint64_t seed, uint64_t first_subsequence, uint32_t n_threads,
                           uint32_t *d_states, const uint32_t *d_matrices, hipStream_t stream);
hipError_t launch_draw_simple(const DrawArgs &a, hipStream_t stream);
hipError_t launch_draw_wave(const DrawArgs &a, bool timed, hipStream_t stream);
hipError_t launch_draw_wave_ship(const DrawArgs &a, bool timed, hipStream_t stream);
// draw_wide.hip: the same path from two waves per SIMD (four orbits per lane in the LONG stage, software-pipelined
// HEAD and REPLAY), so that the scatter of the previous launch fits beside it.  draw_wide_takes: the launches it
// is built for (one-level workspace, one channel, the usual stage split, a carry buffer, whole workgroups of 512
// subsequences); everything else is draw_wave_kernel's.  Same results, own carry format.
bool draw_wide_takes(const DrawArgs &a);
hipError_t launch_draw_wide(const DrawArgs &a, bool timed, hipStream_t stream);
hipError_t launch_draw_wide_ship(const DrawArgs &a, bool timed, hipStream_t stream);
// draw_anti.hip: the anti-Buddhabrot, lockstep = draw_anti_simple_kernel (the definition, lane per thread) or the
// cycle-compressed draw_anti_kernel; a.burning_ship picks the step.  Direct atomics, no workspace, no carry.
hipError_t launch_draw_anti(const DrawArgs &a, bool lockstep, hipStream_t stream);

// The cell grid of the sample plane (draw_cells.h), as the focused and the aimed launch carry it: the list a launch draws
// its samples from, or the mask a probe marks.  All zero: neither, the uniform source and the histogram sink.  FocusArgs
// holds one; AimArgs holds the same seven members itself (why: there).  What reads or fills a grid -- draw_cells.h and the
// two helpers below -- is a template over the block that has the members, `Grid`.
struct CellGrid {
  int level;              // cells of side 2^-level (cells or mask given)
  uint32_t n_cells;       // entries of `cells`
  const uint32_t *cells;  // ascending cell indices row * n + col, n = 4 << level
  uint32_t *mask;         // n * n bits
  double cell_side;       // 2^-level
  double cell_scale;      // 2^-(level + 2): (x + 2) * cell_scale lies in (0, 2^-level]
  double cells_per_unit;  // 2^level
};
// g.level and the three factors made from it (level 0: no grid, the factors stay as they are).
template <class Grid>
void set_grid_level(Grid &g, int level) {
  g.level = level;
  if (level) {
    g.cell_side = ldexp(1.0, -level);
    g.cell_scale = ldexp(1.0, -(level + 2));
    g.cells_per_unit = ldexp(1.0, level);
  }
}
// What no launch takes of a grid: cells and mask together (a probe of a listed stream is not defined), a list without
// entries, a level outside CB_FOCUS_MIN_LEVEL .. CB_FOCUS_MAX_LEVEL when either is given.
template <class Grid>
bool grid_launch_ok(const Grid &g) {
  const bool from_cells = g.cells != nullptr, to_mask = g.mask != nullptr;
  if (from_cells && to_mask) return false;
  if (from_cells && g.n_cells == 0) return false;
  return !(from_cells || to_mask) || (g.level >= CB_FOCUS_MIN_LEVEL && g.level <= CB_FOCUS_MAX_LEVEL);
}

// draw_focus.hip: the focused render (include/cudabrot_amd.h, "Focused render").  A launch is a SOURCE of samples and a
// SINK of accepted orbits:
//   g.cells == null: the uniform source (4 draws per sample over [-2, 2)^2); else the cell list (6 draws per sample);
//   g.mask == null:  the histogram sink (d.hist, every in-canvas point); else the probe's mask (one bit per cell of the
//                    c-plane, set by a sample whose accepted orbit has an in-canvas point; the replay stops there).
// d carries the canvas, the iteration control, the generators, the counters and burning_ship; its workspace, carry and
// interior-map fields are not read.
// hipErrorInvalidValue, nothing launched: what grid_launch_ok refuses of g.
struct FocusArgs {
  DrawArgs d;
  CellGrid g;
};
hipError_t launch_draw_focus(const FocusArgs &a, bool lockstep, hipStream_t stream);

// draw_plot.hip: the plotted renders -- projected ("Projected render" of include/cudabrot_amd.h), Multibrot ("Multibrot
// step"), Julia ("Julia render"), palette ("Palette render") and formula ("Formula step") -- are one launch with a step, a
// source of c and a sink.
//   d        the canvas (the (u, v) window), the iteration control, the generators, the counters and burning_ship; its
//            workspace and carry fields are not read.  d.interior_map (null: none) is read by the product kernel with
//            the Mandelbrot step on a sampled c only: julia == 0, formula == 0, degree == 2, no Burning Ship.
//   p        the matrix P[2][4], rows (u, v), columns (z_re, z_im, c_re, c_im), finite.  Always read.
//   The step: formula != 0 is the code CB_FORMULA_TRICORN .. CB_FORMULA_MAX (0: not a formula), and then degree must be 2
//            and d.burning_ship 0: a formula is a step of its own.  Else degree 2 is the reference's step (d.burning_ship:
//            its Burning Ship variant) and CB_POWER_MIN .. CB_POWER_MAX the Multibrot step z <- z^degree + c, which has no
//            Burning Ship variant.
//   The source of c: julia == 0 samples c from the stream (z_0 = c); julia != 0 takes the fixed c = (c[0], c[1]), both in
//            [-2, 2], and the sample of the stream is z_0.  c is read only when julia != 0.
//   The sink: palette == 0 adds 1 per point to the one plane d.hist; palette != 0 makes d.hist three planes plane_pixels
//            counters apart and lut the table on the device, d.max_iter entries -- which must be 1 ..
//            CB_PALETTE_MAX_ENTRIES -- of which entry k carries the weights of an orbit with escape index k.  lut and
//            plane_pixels are read only when palette != 0.
// hipErrorInvalidValue, nothing launched: a degree outside {2, CB_POWER_MIN .. CB_POWER_MAX}; a degree other than 2 or
// the Burning Ship beside a formula; the Burning Ship beside a degree other than 2; julia with a c outside [-2, 2], a NaN
// included; palette with a null table or a max_iter outside 1 .. CB_PALETTE_MAX_ENTRIES; a formula code above
// CB_FORMULA_MAX or below 0.  lockstep: the definition, one lane per reference thread -- the formula's kernel, else the
// palette's, else the Julia render's, else the Multibrot step's, else the projected render's.
struct PlotArgs {
  DrawArgs d;
  double p[8];
  int degree;
  double c[2];
  int julia;
  const uint32_t *lut;
  unsigned long long plane_pixels;
  int formula;
  int palette;
};
hipError_t launch_draw_plot(const PlotArgs &a, bool lockstep, hipStream_t stream);

// draw_depth.hip: the depth render ("Depth render" of include/cudabrot_amd.h) -- a plotted launch without a table whose
// visited points are binned along a third row as well, into `slices` planes of the histogram.
//   p        the launch of draw_plot.hip it extends: canvas, matrix, step and source of c as there; palette must be 0 and
//            lut null.  p.d.hist is `slices` planes plane_pixels counters apart.
//   row      the depth row D, columns (z_re, z_im, c_re, c_im), finite.
//   min, delta, inv_delta, pow2   the depth window's lower bound and its step (max - min) / slices, made on the host as
//            DrawArgs::delta_imag is; pow2 != 0: delta is a power of two and inv_delta its exact reciprocal.
//   slices   N, 1 .. CB_DEPTH_MAX_SLICES.
//   plane_pixels   w * h.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_plot refuses of p, a table, slices out of range, a delta
// that is not positive, a plane_pixels that is not w * h.  lockstep: the definition, one lane per reference thread.
struct DepthArgs {
  PlotArgs p;
  double row[4];
  double min, delta, inv_delta;
  int pow2, slices;
  unsigned long long plane_pixels;
};
hipError_t launch_draw_depth(const DepthArgs &a, bool lockstep, hipStream_t stream);

// draw_depth_palette.hip: the depth-palette render ("Depth-palette render" of include/cudabrot_amd.h) -- a depth launch
// whose slice looks a colour up: a point on the canvas and in depth adds the three weights of lut[s] to its pixel of three
// planes.
//   d        the depth launch it extends, d.p.palette 0 and d.p.lut null as there (the table is not the palette render's:
//            it is indexed by the slice).  d.p.d.hist is three planes.
//   lut      the table on the device, d.slices entries in the palette's entry format.
//   plane_pixels   w * h: the distance between the three planes.
// n_entries: the table's length, which the kernels never see.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_depth refuses of d (but the table), a null table, n_entries
// != d.slices, a plane_pixels that is not w * h.  lockstep: the definition, one lane per reference thread.
struct DepthPaletteArgs {
  DepthArgs d;  // first: the kernels read it through draw_depth.h's fresh_depth_args
  const uint32_t *lut;
  unsigned long long plane_pixels;
};
hipError_t launch_draw_depth_palette(const DepthPaletteArgs &a, uint32_t n_entries, bool lockstep, hipStream_t stream);

// draw_frames.hip: the frames render ("Frames render" of include/cudabrot_amd.h) -- a plotted launch without a table whose
// visited points are plotted with n_frames matrices instead of one, each into a plane of its own.
//   p        the launch of draw_plot.hip it extends: canvas, step and source of c as there; palette must be 0 and lut null;
//            p.p is not read.  p.d.hist is n_frames planes plane_pixels counters apart.
//   frames   the matrices on the device, n_frames x 8 doubles, each P[2][4] as PlotArgs::p, finite (the caller's word).
//   n_frames F, 1 .. CB_FRAMES_MAX.
//   plane_pixels   w * h.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_plot refuses of p, a table, null matrices, n_frames out of
// range, a plane_pixels that is not w * h, n_frames * h above INT_MAX.  lockstep: the definition, one lane per reference
// thread.
struct FramesArgs {
  PlotArgs p;
  const double *frames;
  int n_frames;
  unsigned long long plane_pixels;
};
hipError_t launch_draw_frames(const FramesArgs &a, bool lockstep, hipStream_t stream);

// draw_phoenix.hip: the Phoenix render ("Phoenix render" of include/cudabrot_amd.h) -- a projected or Julia launch whose
// step has memory: z_{n+1} = z_n^2 + c + p z_{n-1}.
//   plot     the launch of draw_plot.hip it extends: canvas, matrix and source of c as there; degree must be 2, formula,
//            d.burning_ship and palette 0 and lut null.  d.interior_map is not read: nothing is rejected or retired as
//            drawn.
//   p        the parameter (p_re, p_im), both in [-2, 2].
// hipErrorInvalidValue, nothing launched: whatever launch_draw_plot refuses of plot, a degree other than 2, a formula, the
// Burning Ship, a table, a p outside [-2, 2], a NaN included.  lockstep: the definition, one lane per reference thread.
struct PhoenixArgs {
  PlotArgs plot;
  double p[2];
};
hipError_t launch_draw_phoenix(const PhoenixArgs &a, bool lockstep, hipStream_t stream);

// draw_bounded.hip: the bounded render ("Bounded render" of include/cudabrot_amd.h) -- a plotted launch that plots the
// orbits that do NOT escape, z_1 .. z_M, as the anti-Buddhabrot records them: nothing rejected, d.min_iter and
// d.interior_map not read, one plane.  Step and source of c as launch_draw_plot's; palette must be 0 and lut null.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_plot refuses of a, a table.  lockstep: the definition, one
// lane per reference thread, every point with weight 1; else the cycle-compressed product kernel.
hipError_t launch_draw_bounded(const PlotArgs &a, bool lockstep, hipStream_t stream);

// draw_aim.hip: the aimed render ("Aimed render" of include/cudabrot_amd.h) -- an un-aimed render (a projected or Julia
// launch of draw_plot.hip without a table, or a bounded launch of draw_bounded.hip) behind the focused render's source and
// in front of its sink:
//   p        the un-aimed launch: canvas, matrix, step and source of c as there; palette must be 0 and lut null.
//            p.d.interior_map is read by the escaping kind with the Mandelbrot step on a sampled c only.
//   bounded  0: the escaping orbits that pass the accept filter (launch_draw_plot); else the orbits that do not escape
//            (launch_draw_bounded).
//   cells == null: the uniform source (4 draws per sample over [-2, 2)^2); else the cell list (6 draws per sample),
//            the cells those of the SAMPLE plane: c when c is sampled, z_0 when c is fixed;
//   mask == null:  the histogram sink (p.d.hist, what the un-aimed launch adds); else the probe's mask (one bit per
//            cell, set by a sample whose plotted orbit has an in-canvas point; the replay stops there, p.d.hist is not
//            read).
//   The grid's members are CellGrid's, with its meanings, written out: behind the int `bounded` a nested CellGrid would
//   start four bytes later than `level` does here, the compiler would fetch level, n_cells and cells with one scalar load
//   where it now needs two, and the 53 kernels that read them would come out with other scalar registers and eight bytes
//   shorter.  Measured, the Mandelbrot-step draw was 1.5 % slower that way, beyond the spread of its runs.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_plot refuses of p, a table, what grid_launch_ok refuses of
// the grid.  lockstep: the definition, one lane per reference thread, every point with weight 1.
struct AimArgs {
  PlotArgs p;
  int bounded;
  int level;
  uint32_t n_cells;
  const uint32_t *cells;
  uint32_t *mask;
  double cell_side, cell_scale, cells_per_unit;
};
hipError_t launch_draw_aim(const AimArgs &a, bool lockstep, hipStream_t stream);

// draw_periods.hip: the period-palette render ("Period-palette render" of include/cudabrot_amd.h) -- a bounded launch whose
// bounded orbits look a colour up by the period of the cycle they fall onto: each of the M points adds the three weights of
// lut[period] to its pixel of three planes.
//   p        the bounded launch it extends, p.palette 0 and p.lut null as there (the table is not the palette render's: it
//            is indexed by the period).  p.d.hist is three planes.
//   lut      the table on the device, n_entries entries in the palette's entry format, 2 .. CB_PERIOD_MAX_ENTRIES.
//   eps      the tolerance of the return test, finite and >= 0.
//   plane_pixels   w * h: the distance between the three planes.
// hipErrorInvalidValue, nothing launched: whatever launch_draw_bounded refuses of p, a null table, n_entries out of range,
// an eps that is negative, infinite or a NaN, a plane_pixels that is not w * h.  lockstep: the definition, one lane per
// reference thread; else the cycle-compressed product kernel with its scheduled search.
struct PeriodArgs {
  PlotArgs p;
  const uint32_t *lut;
  int n_entries;
  double eps;
  unsigned long long plane_pixels;
};
hipError_t launch_draw_periods(const PeriodArgs &a, bool lockstep, hipStream_t stream);

// How an image is exposed: against its largest counter, against the white point of a clip of `clip_percent` ("White
// clip" of include/cudabrot_amd.h), by the rank of its counters ("Equalised image"), or by their rank in the tiles of a
// grid ("Locally equalised image": the image is `planes` planes, one above the other, that share the tiles' tables).
struct Exposure {
  enum Kind { kPlain, kWhiteClip, kEqualized, kLocalEqualized } kind;
  double clip_percent;  // kWhiteClip's
  int planes = 1, tiles_x = 0, tiles_y = 0;  // kLocalEqualized's
  uint32_t clip_q = 0;
};
// What exposing found: max always; white, lit and clipped under a white clip; lit, keys and levels equalised; lit,
// lit_tiles and moved locally equalised; 0 else.
struct Exposed {
  uint64_t max, white, lit, clipped, keys, levels, lit_tiles = 0, moved = 0;
};
// tonemap.hip: finds the top of w x h device counters as `how` says, maps them into big-endian u16 -- the table or the
// thresholds, as `mode` (CB_TONE_*) and the top choose; an equalised image has one form -- and reports: what
// cb_tone_map_device, cb_tone_map_device_white and cb_tone_map_device_equalized do, and what a renderer keeps for
// cb_renderer_last_white, cb_renderer_last_equalize and cb_renderer_last_local_equalize.  *found is written on success
// only.  Synchronises `stream`.
int tone_map_exposed(const unsigned long long *hist, int w, int h, double gamma, int mode, const Exposure &how,
                     uint16_t *d_gray_be, Exposed *found, hipStream_t stream);
// exposure.hip: cb_white_count_device, and the largest counter beside its three numbers (max_out may be null).
int white_count_device(const unsigned long long *hist, unsigned long long n, double clip_percent, uint64_t *white_out,
                       uint64_t *lit_out, uint64_t *clipped_out, uint64_t *max_out, hipStream_t stream);
// equalize.hip: cb_equalize_bins_device, and the lookup of n counters' keys in a host table of CB_EQUALIZE_KEYS values.
int equalize_bins_device(const unsigned long long *hist, unsigned long long n, uint64_t *bins_out_host, uint64_t *lit_out,
                         uint64_t *max_out, hipStream_t stream);
int equalize_map_device(const unsigned long long *hist, unsigned long long n, const uint16_t *table_host, uint16_t *d_gray_be,
                        hipStream_t stream);
// tonemap.hip: the largest of n device counters.  Synchronises `stream`.
int hist_max_device(const unsigned long long *hist, unsigned long long n, uint64_t *max_out, hipStream_t stream);
// equalize_local.hip: what cb_local_equalize_bins_device (bins_out_host: tx * ty rows of CB_EQUALIZE_KEYS) and
// cb_tone_map_device_local_equalized (d_gray_be) do; either output may be null.
int local_equalize_device(const unsigned long long *hist, int w, int h, int planes, int tx, int ty, uint32_t clip_q,
                          double gamma, uint64_t *bins_out_host, uint16_t *d_gray_be, Exposed *found, hipStream_t stream);

// Steps per chunk of the LONG stage; the stage split is chosen so that no chunk straddles min_iter.
// The exact-periodicity check compares z with a saved point at chunk boundaries only, so a cycle of period
// p is seen p / gcd(p, chunk) chunks after the save.  The periods that matter are mostly multiples of 3
// (by area of the set outside the cardioid and the period-2 disc: 3, 4, 6, 12, 9, 5, 8, 15, 10 ...), so
// 30 = 2 * 3 * 5 finds them sooner than 32: 9 % fewer executed iterations at C3, the draw launch 5 %
// shorter (24 and 36 measured too).  With the sparse escape tests (draw_wave.hip, iterate_chunk2_sparse) a
// chunk of 30 had become so short that the bookkeeping between chunks was a sixth of it: 60 = 4 * 3 * 5
// executes 5 % more iterations and is 5 % faster (measured).
constexpr int kChunk = 60;
void plan_stages(int max_iter, int min_iter, int *head_steps, int *mid_steps);

}  // namespace cb
