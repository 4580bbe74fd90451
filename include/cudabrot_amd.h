/*
 * cudabrot_amd.h -- C ABI of the MI355X-native Buddhabrot hot path (libcudabrot_amd.so).
 *
 * The reference (yalue/cudabrot, one file: cudabrot.cu) has no FFI or plugin interface; its only
 * internal boundary is the pair of kernel launches its host driver makes (last
 * row).  The entry points below are exactly that boundary, as a C ABI: plain pointers and sizes, no
 * C++ or torch types.  Each cites the reference interface it replaces.
 *
 * Conventions
 *  - every function returns 0 on success or a hipError_t value (>0); cb_error_string() names it,
 *    the way the reference prints cudaGetErrorString (cudabrot.cu:134-141);
 *  - pointers named d_* are DEVICE pointers on the current HIP device, `stream` is a hipStream_t
 *    passed as void* (NULL = the default stream); launches are asynchronous on that stream;
 *  - the library never falls back to the CPU: without a usable HIP device every call fails.
 */
#ifndef CUDABROT_AMD_H_
#define CUDABROT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CB_ABI_VERSION 1

/* Reference constants (cudabrot.cu:20,23,34,37). */
#define CB_DEFAULT_BLOCK_SIZE 512
#define CB_DEFAULT_BLOCK_COUNT 512
#define CB_DEFAULT_THREADS (CB_DEFAULT_BLOCK_SIZE * CB_DEFAULT_BLOCK_COUNT)
#define CB_SAMPLES_PER_THREAD 50
#define CB_DEFAULT_RNG_SEED 1337ull

/* `Pixel` (cudabrot.cu:43), widened to 64 bits as BASELINE.json's north_star asks: identical to the
 * reference's uint32_t counts whenever no count reaches 2^32. */
typedef uint64_t cb_pixel;

/* `FractalDimensions` (cudabrot.cu:46-58): same fields, same order, same layout (56 bytes). */
typedef struct {
  int w;
  int h;
  double min_real;
  double min_imag;
  double max_real;
  double max_imag;
  double delta_real;
  double delta_imag;
} cb_fractal_dimensions;

/* `IterationControl` (cudabrot.cu:62-67). */
typedef struct {
  int max_escape_iterations;
  int min_escape_iterations;
} cb_iteration_control;

/* Exact workload counters, accumulated on the device; the reference has none. */
typedef struct {
  uint64_t samples;        /* starting points drawn (4 XORWOW outputs each)              */
  uint64_t rejected;       /* inside the main cardioid / period-2 bulb (cudabrot.cu:398) */
  uint64_t never_escaped;  /* IterateMandelbrot returned max (cudabrot.cu:407)           */
  uint64_t too_fast;       /* escaped before min_escape_iterations (cudabrot.cu:408)     */
  uint64_t recorded;       /* orbits replayed (cudabrot.cu:412)                          */
  uint64_t iterate_steps;  /* z<-z^2+c iterations of IterateMandelbrot (cudabrot.cu:326),
                              as the reference would execute them                        */
  uint64_t replay_steps;   /* iterations of IterateAndRecord (cudabrot.cu:352)           */
  uint64_t increments;     /* histogram increments (cudabrot.cu:312)                     */
  uint64_t skipped_steps;  /* part of iterate_steps NOT executed: the orbit was found to be
                              exactly periodic, or its cell is proven never-escaping (the
                              interior map)                                               */
  uint64_t status;         /* 0 = ok; nonzero = internal invariant violated (CB_STATUS_*) */
  /* CB_KERNEL_TIMED only (else 0): shader-clock cycles summed over waves, per stage and in total */
  uint64_t cycles_head, cycles_long, cycles_replay, cycles_total;
  /* CB_KERNEL_TIMED only, 100 MHz constant clock, LAST launch only meaningful if counters were zeroed
   * before it: ~(earliest wave start), latest wave end, sum of wave lifetimes */
  uint64_t rt_not_first_start, rt_last_end, rt_wave_life_sum;
} cb_counters;

#define CB_STATUS_QUEUE_OVERFLOW 1u
#define CB_STATUS_REPLAY_RUNAWAY 2u
#define CB_STATUS_INTERIOR_MAP 4u /* a sample of a cell proven never-escaping (interior map) escaped */
#define CB_STATUS_CARRY_FOREIGN 8u /* the carry buffer holds work of the OTHER draw kernel (another workspace size or
                                      none picks another kernel: see cb_draw_buddhabrot): it was not resumed */
/* Returned (instead of a hipError_t) by cb_renderer_finish and by everything that reads a renderer's histogram
 * or image when cb_counters.status is nonzero: a draw kernel saw one of its internal invariants broken and has
 * lost samples, so the histogram is not a result.  cb_renderer_read_counters still succeeds and shows the flags. */
#define CB_ERROR_KERNEL_INVARIANT 100001

/* Kernel variants of cb_draw_buddhabrot. */
#define CB_KERNEL_DEFAULT 0 /* wave-scheduled four-stage kernel (the product path)                */
#define CB_KERNEL_SIMPLE 1  /* one lane = one reference thread, lock-step; a validation baseline  */
#define CB_KERNEL_TIMED 2   /* the default kernel with per-stage s_memtime stamps (diagnostic build) */
#define CB_KERNEL_FULL_ITERATE 3 /* the default kernel without the exact-periodicity early-out: every
                                    sample is iterated to max_iter as the reference does (same result;
                                    for measuring the iterate loop against the fp64 roofline)        */

/* Fused multi-channel renders: at most this many (max, min) windows per launch. */
#define CB_MAX_CHANNELS 4

/* OR-ed into a kernel variant: the reference's RENDER_BURNING_SHIP build (cudabrot.cu:15-17 -- there a
 * compile-time switch): |real|, |imag| before every step and no cardioid / bulb shortcut. */
#define CB_KERNEL_FLAG_BURNING_SHIP 0x100

/* OR-ed into a kernel variant, with a carry buffer: this launch also completes every orbit in flight
 * (its own and the carried ones) instead of leaving them for the next launch -- the last launch of a
 * render.  A launch with samples_per_thread = 0 does only that. */
#define CB_KERNEL_FLAG_DRAIN 0x200

/* OR-ed into CB_KERNEL_DEFAULT (the cycle-compressed product kernel) or CB_KERNEL_SIMPLE (the lock-step kernel), with or
 * without CB_KERNEL_FLAG_BURNING_SHIP: the ANTI-Buddhabrot, the orbits of the samples that do NOT escape.
 * Normative:
 *   samples: the same stream as a normal render (same subsequences, 4 XORWOW draws per sample); the step is the
 *   canonical fp64 step of the variant.  With z_0 = c, z_k = step(z_{k-1}) and M = max_escape_iterations, a sample
 *   ESCAPES if |z_k|^2 > 4 for some 1 <= k <= M.  No cardioid / bulb rejection, no interior map.
 *   recorded: a non-escaping sample adds z_1 .. z_M, M points, each binned as a normal replay bins its points; an
 *   escaping sample adds nothing.  min_escape_iterations is ignored.  M <= 0 tests nothing and adds no point: every
 *   sample counts as not escaping (never_escaped = recorded = samples) and the step counters stay 0.
 *   counters: samples as usual; rejected 0; never_escaped = recorded = the non-escaping samples; too_fast = the
 *   escaping samples; iterate_steps = sum of k over the escapers + M per non-escaping sample (what the definition
 *   executes); replay_steps = M * recorded; increments = the weighted in-canvas increments (what the histogram gains);
 *   skipped_steps = the part of iterate_steps + replay_steps not executed.  All but skipped_steps and the timing fields
 *   are identical between the two kernels.
 *   cycle compression (the product kernel): if z_1 .. z_n were tested not escaping and z_n == z_s bit for bit in both
 *   components, 1 <= s < n <= M, p = n - s, the orbit never escapes and its M points are z_1 .. z_{s-1} with weight 1
 *   and z_{s+j}, 0 <= j < p, with weight floor((M - s - j) / p) + 1: the same histogram, bit for bit.
 * An anti launch ignores d_workspace and d_carry and is complete when it ends; cb_draw_buddhabrot_channels refuses it
 * (hipErrorInvalidValue), as cb_draw_buddhabrot does with any other base variant. */
#define CB_KERNEL_FLAG_ANTI 0x400

/* ---- Multibrot step: z^d + c on the projected render ----------------------------- *
 *
 * CB_KERNEL_POWER(d), OR-ed into CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, replaces the step of a PROJECTED render
 * ("Projected render" below) by z <- z^d + c.  Field 0 means the step as without it.  Normative:
 *
 *   Degree.  CB_POWER_MIN = 3 <= d <= CB_POWER_MAX = 8.
 *
 *   Step.  One step from z = (r, i) with sample c = (cr, ci) is IEEE fp64; each fma is one rounding and nothing else is
 *   contracted:
 *       wr = r; wi = i
 *       repeat d-1 times, in this order:
 *           t  = wi * i            nr = fma(wr, r, -t)
 *           s  = wi * r            ni = fma(wr, i,  s)
 *           wr = nr; wi = ni
 *       r' = cr + wr;  i' = ci + wi
 *       m  = fma(i', i', r' * r')          escape: m > 4.0
 *   The power is d - 1 multiplications by z, left to right.  Addition chains such as (z^2)^2 are faster but round
 *   differently, so they are not this definition.
 *
 *   Everything else is the projected render's: the normal sample stream (4 XORWOW draws per sample, z_0 = c),
 *   IterateMandelbrot's loop shape (k = index of the first escaping z_{k+1}, or max), the accept filter min <= k < max,
 *   the replay of z_1 ... z_{k+1}, the projection P[2][4] with its four fused operations per point, and the binning.  As
 *   for the Burning Ship there is no cardioid or bulb rejection (rejected = 0) and no interior map.  Counters keep their
 *   normal meaning; skipped_steps is the executed-work discount.
 *
 *   Every visited point is finite: the point before an escaping one has |z|^2 <= 4, so the escaping point has
 *   |z| <= 2^8 + |c|.  The plain Multibrot image is therefore the identity projection P = {{1,0,0,0},{0,1,0,0}}, which
 *   cannot move a bin ("Projected render", Identity).
 *
 * Accepted by cb_draw_buddhabrot_projected and by cb_renderer_render_passes / cb_renderer_prepare on a projected
 * renderer.  hipErrorInvalidValue, with nothing launched or written: a field value of 1, 2 or 9 ... 15; a degree together
 * with CB_KERNEL_FLAG_BURNING_SHIP, CB_KERNEL_FLAG_ANTI or a base variant other than the two above; a degree given to
 * cb_draw_buddhabrot, cb_draw_buddhabrot_channels, cb_focus_probe, cb_draw_buddhabrot_focus, cb_renderer_set_focus, or to
 * cb_renderer_render_passes on a renderer without a projection.
 * Two kernels (draw_plot.hip): CB_KERNEL_DEFAULT, one instance per degree with the step unrolled, lanes refilled from
 * their own subsequence, with the exact-periodicity early-out; CB_KERNEL_SIMPLE, the definition in lock-step with the
 * degree a run-time argument.  Identical histograms, generator states and counters (but skipped_steps).
 * The -s buffer records the degree no more than it records the plane: resuming a buffer with another degree adds two
 * different images, and nothing can notice. */
#define CB_POWER_MIN 3
#define CB_POWER_MAX 8
#define CB_KERNEL_POWER(d) ((d) << 12)
#define CB_KERNEL_POWER_MASK 0xF000

/* ---- Formula step: tricorn, Celtic and kin on the projected render ----------------- *
 *
 * CB_KERNEL_FORMULA(f), OR-ed into CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, replaces the step of a PROJECTED render
 * ("Projected render" below), of a JULIA render or of a PALETTE render by another member of the quadratic family whose
 * members differ from the reference's step by a sign or an absolute value.  Field 0 means the step as without it.  This
 * is the project's own definition: sign conventions differ between programs, and these are ours.  Normative:
 *
 *   Code.  CB_FORMULA_TRICORN = 1 <= f <= CB_FORMULA_MAX = 5.
 *
 *   Step.  One step from z = (r, i) with c = (cr, ci) is IEEE fp64; each fma is one rounding and nothing else is
 *   contracted; negation and fabs are exact:
 *       ii = i * i
 *       t  = fma(r, r, -ii)
 *       nr, ni by the code:
 *         code  name              nr             ni
 *         1     tricorn           cr + t         fma(-(r + r), i, ci)                         (the Mandelbar)
 *         2     celtic            cr + fabs(t)   fma(r + r, i, ci)
 *         3     buffalo           cr + fabs(t)   fma(fabs(r) + fabs(r), fabs(i), ci)          (the Burning Ship's cross term)
 *         4     perpendicular     cr + t         fma(-(fabs(r) + fabs(r)), i, ci)
 *         5     celtic-tricorn    cr + fabs(t)   fma(-(r + r), i, ci)                         (the Celtic Mandelbar)
 *       r' = nr;  i' = ni
 *       m  = fma(ni, ni, nr * nr)          escape: m > 4.0
 *   With nr = cr + t and ni = fma(r + r, i, ci) this is the reference's step, which has no code.
 *
 *   Everything else is a Multibrot render's ("Multibrot step"): a projected render, on the identity matrix unless one is
 *   given; the normal sample stream (4 XORWOW draws per sample, z_0 = c); IterateMandelbrot's loop shape (k = index of
 *   the first escaping z_{k+1}, or max); the accept filter min <= k < max; the replay of z_1 ... z_{k+1}; the projection
 *   P[2][4] with its four fused operations per point; the binning.  No cardioid or bulb rejection (rejected = 0) and no
 *   interior map (cb_debug_interior_map_level() == 0).  Counters keep their normal meaning; skipped_steps is the
 *   executed-work discount of the product kernel.
 *
 *   Every visited point is finite: a visited point follows a point with |z|^2 <= 4 (z_0 = c or a point that passed the
 *   test), and |t| <= |z|^2, 2 |r| |i| <= |z|^2, so |nr| <= |cr| + 4 and |ni| <= |ci| + 4 up to rounding: |z'| <= 4 +
 *   |c| <= 4 + 2 sqrt(2).  The identity projection cannot move a bin ("Projected render", Identity).
 *
 *   With a fixed c (cb_draw_buddhabrot_julia): the fixed c goes into the same step, and everything else is under "Julia
 *   render"'s rules -- the sample is z_0, |z_0|^2 may exceed 4 and z_1 is then finite all the same (|z_0| <= 2 sqrt(2)).
 *   With a table (cb_draw_buddhabrot_palette): under "Palette render"'s rules, for a sampled c or a fixed one.
 *
 * Accepted by cb_draw_buddhabrot_projected, cb_draw_buddhabrot_julia, cb_draw_buddhabrot_palette and by
 * cb_renderer_render_passes on a projected, Julia or palette renderer.  hipErrorInvalidValue, with nothing launched or
 * written: a field value of 6 ... 15; a code together with CB_KERNEL_FLAG_BURNING_SHIP, CB_KERNEL_FLAG_ANTI,
 * CB_KERNEL_FLAG_DRAIN, CB_KERNEL_POWER(d) or a base variant other than the two above; a code given to
 * cb_draw_buddhabrot, cb_draw_buddhabrot_channels, cb_focus_probe, cb_draw_buddhabrot_focus, cb_renderer_set_focus, or to
 * cb_renderer_render_passes on a plain, channel or focused renderer.
 * Two kernels (draw_plot.hip): CB_KERNEL_DEFAULT, one instance per code, per source of c (sampled, fixed) and per
 * sink (one plane, the palette's three), lanes refilled from their own subsequence, with the exact-periodicity
 * early-out; CB_KERNEL_SIMPLE, the definition in lock-step with code, source and sink run-time arguments.  Identical
 * histograms, generator states and counters (but skipped_steps).
 * The -s buffer records the formula no more than it records the plane. */
#define CB_FORMULA_TRICORN 1
#define CB_FORMULA_CELTIC 2
#define CB_FORMULA_BUFFALO 3
#define CB_FORMULA_PERPENDICULAR 4
#define CB_FORMULA_CELTIC_TRICORN 5
#define CB_FORMULA_MAX 5
#define CB_KERNEL_FORMULA(f) ((f) << 16)
#define CB_KERNEL_FORMULA_MASK 0xF0000

/* Returned (instead of a hipError_t) by cb_renderer_set_focus when the probe marked no cell: no sample of the probe has
 * an accepted orbit that enters the canvas, so a focused render would have nothing to sample from. */
#define CB_ERROR_FOCUS_EMPTY 100002
/* cb_renderer_set_aim: the probe marked no cell ("Aimed render"). */
#define CB_ERROR_AIM_EMPTY 100003

/* RecomputePixelDeltas (cudabrot.cu:505-527).  Returns 1 and fills delta_* if the canvas is valid,
 * else 0 and, if msg is not NULL, *msg points at the reference's message for the failed check. */
int cb_recompute_pixel_deltas(cb_fractal_dimensions *dims, const char **msg);

/* Bytes of device memory cb_initialize_rng / cb_draw_buddhabrot need at d_states for n_threads
 * generator states (replaces `block_size * block_count * sizeof(curandState_t)`, cudabrot.cu:177-178).
 * Layout: six uint32 planes [x0 | x1 | x2 | x3 | x4 | d], each n_threads long. */
size_t cb_rng_state_bytes(uint32_t n_threads);

/* InitializeRNG<<<...>>>(seed, states) (cudabrot.cu:146-149,179): state t becomes the XORWOW
 * generator rocrand_init(seed, first_subsequence + t, 0).  The reference always passes
 * first_subsequence = 0; rank r of a multi-GPU run passes r * n_threads. */
int cb_initialize_rng(uint64_t seed, uint64_t first_subsequence, uint32_t n_threads, void *d_states,
                      void *stream);

/* Suggested size of the scatter workspace of cb_draw_buddhabrot for launches of this shape (0 if the canvas
 * cannot use one: more than 262144 tiles of 128x128 pixels, or a side above 65536).  Any size works:
 * increments that do not fit are added with direct atomics, the result is the same. */
size_t cb_scatter_workspace_bytes(const cb_fractal_dimensions *dims, uint32_t n_threads,
                                  uint32_t samples_per_thread);
/* ... of cb_draw_buddhabrot_channels with n_channels planes (their tiles are sorted as one canvas). */
size_t cb_scatter_workspace_bytes_channels(const cb_fractal_dimensions *dims, int n_channels, uint32_t n_threads,
                                           uint32_t samples_per_thread);

/* DrawBuddhabrot<<<block_count, block_size>>>(dimensions, data, iterations, states)
 * (cudabrot.cu:379-414,485-486) for n_threads threads, samples_per_thread samples each (the
 * reference: 50 per launch; k reference passes in one launch = 50*k).  Adds to d_hist (w*h
 * cb_pixel, row-major, row 0 = min_imag), advances d_states, and adds to d_counters (may be NULL).
 * Without a workspace (d_workspace NULL) every increment is a device-scope atomic on d_hist (the
 * reference's += of cudabrot.cu:312, made atomic) and d_hist is complete when the launch is.
 * With one, the increments that fit are DEFERRED: the kernel streams the visited pixels into the
 * workspace and the caller must then run cb_flush_scatter on the same workspace (stream-ordered
 * after this call) before it reads d_hist or reuses the workspace; what does not fit is added
 * atomically at once, so the sum is the same for any workspace size.
 * d_carry (may be NULL: then the launch completes every sample it draws, like the reference's) is
 * cb_carry_bytes(n_threads) of device memory, zeroed before the first call, that carries orbits
 * still in flight from one launch to the next: finishing the deepest orbits of a launch takes
 * hundreds of iterations with almost every lane idle, so with a carry buffer the launch stops when
 * its samples are drawn.  A final call with samples_per_thread == 0 (followed by its
 * cb_flush_scatter) completes the carried work; only then do d_hist and d_counters account for
 * every sample drawn.  Same geometry, iteration control, kernel variant AND workspace (its size, or none)
 * for all calls sharing a carry buffer: the library has two draw kernels with carry records of their own and
 * picks one by the shape of the launch, the workspace included.  A call that finds the other kernel's work
 * in the buffer does not resume it and says so: cb_counters.status gets CB_STATUS_CARRY_FOREIGN (cb_renderer
 * keeps all of this consistent by itself). */
int cb_draw_buddhabrot(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                       const cb_iteration_control *iterations, void *d_states, uint32_t n_threads,
                       uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                       void *d_workspace, size_t workspace_bytes, void *d_carry, void *stream);

/* Bytes of the carry buffer of cb_draw_buddhabrot for n_threads threads. */
size_t cb_carry_bytes(uint32_t n_threads);

/* Second half of the scatter: partitions the pixel stream a cb_draw_buddhabrot call left in
 * d_workspace by 128x128-pixel tile (sorts of regions of 32768 entries) and adds every tile to d_hist from an LDS
 * histogram with coalesced atomics.  Same dims, n_threads, d_workspace and workspace_bytes as that
 * call.  A no-op for a workspace the draw call could not use.  Precondition: the workspace was last written by
 * a cb_draw_buddhabrot call with these arguments (a call that launches nothing -- no samples, nothing to
 * drain -- leaves an empty stream); flushing a workspace no draw call has touched is undefined.
 * Meant to run on ANOTHER stream than the next draw call, beside it (two workspaces, as cb_renderer does): its kernels
 * fit the CUs beside the two-waves-per-SIMD draw kernel.  The first of them is one wave that sleeps 40 us, so that a
 * draw launch released by the same event reaches the empty CUs first (otherwise the region
 * sort cannot be resident beside the draw's waves and runs after them). */
int cb_flush_scatter(const cb_fractal_dimensions *dims, cb_pixel *d_hist, uint32_t n_threads,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Fused multi-channel render ---------------------------------------------- *
 *
 * The reference's colour recipe (generate_hires_color_image.sh:27-59) runs the program once per
 * channel with different -m / -c.  All runs draw the same sample stream, so one pass can serve them:
 * every sample is iterated once up to the largest max, and its orbit is replayed once into every
 * channel j whose window windows[j].min <= k < windows[j].max holds the escape index k; the planes are
 * then sorted and accumulated together, as one taller canvas.  d_hist is
 * n_channels planes of w*h counters, plane j = what cb_draw_buddhabrot would add with windows[j].
 * The wave-scheduled kernel only (variant flags as above); cb_flush_scatter_channels after each
 * launch that was given a workspace (sized by cb_scatter_workspace_bytes_channels).
 * Counters of a fused launch: samples, rejected, never_escaped (against the largest max) and
 * iterate_steps as for one run with the largest max; too_fast = orbits that escaped but whose index
 * lies in no window; recorded = orbits in at least one window; replay_steps counts every replay (a first,
 * unrecorded one finds the escape index, then one per channel the orbit belongs to); increments = the
 * histogram increments of all planes together. */
int cb_draw_buddhabrot_channels(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                const cb_iteration_control *windows, int n_channels, void *d_states,
                                uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                int kernel_variant, void *d_workspace, size_t workspace_bytes,
                                void *d_carry, void *stream);
int cb_flush_scatter_channels(const cb_fractal_dimensions *dims, cb_pixel *d_hist, int n_channels,
                              uint32_t n_threads, void *d_workspace, size_t workspace_bytes,
                              void *stream);

/* ---- Focused render: a cropped canvas sampled only from the cells that reach it -- *
 *
 * A render of a small window wastes almost every sample: samples are drawn over [-2, 2]^2 and few of their orbits enter
 * the window.  A focused render first PROBES which cells of the c-plane hold samples whose orbits reach the canvas, and
 * then draws its samples from those cells only.  The project's own definition (the reference has none).  Normative:
 *
 *   Grid.  Level L, CB_FOCUS_MIN_LEVEL <= L <= CB_FOCUS_MAX_LEVEL.  Cells of side 2^-L over [-2, 2)^2, n = 4 * 2^L
 *   cells per side; cell (row, col) has the corner lo_re = -2 + col * 2^-L, lo_im = -2 + row * 2^-L (exact) and the
 *   index row * n + col.  A MASK is n * n bits in uint32_t words: bit (index & 31) of word (index >> 5).
 *
 *   Probe.  A normal launch on the normal sample stream (4 XORWOW draws per sample, the same cardioid / bulb rejection,
 *   iterate, accept filter min <= k < max, replay and binning as cb_draw_buddhabrot), except that nothing is added to a
 *   histogram: a sample whose accepted orbit has AT LEAST ONE in-canvas point sets the bit of the cell that holds its c,
 *   col = (int)((re + 2) * 2^L), row = (int)((im + 2) * 2^L), both exact; re = 2 exactly, which the sample stream can
 *   return, is clamped to n - 1.  The mask is a union of bits and so independent of the schedule.  The replay stops at
 *   the first in-canvas point.  Counters as a normal launch, except: recorded = the samples that set a bit (newly or
 *   not), replay_steps = the replay steps up to and including that first point (all of them for an orbit that never
 *   enters), increments = 0.
 *
 *   Cell list.  The mask dilated by d cells in the Chebyshev metric (d >= 0, clipped at the grid's edge), then the set
 *   cells in ascending index order: cells[0 .. n_cells).
 *
 *   Focused draw.  Thread t consumes its subsequence SIX draws per sample, in this order: a = next(), b = next();
 *   j = (((uint64_t)a << 32 | b) * n_cells) >> 64 (the high half of the 128-bit product); cell = cells[j];
 *   x = the next coordinate of the normal stream, y = the one after (two draws each, values in (-2, 2]);
 *   re = lo_re(cell) + (x + 2.0) * 2^-(L+2), im = lo_im(cell) + (y + 2.0) * 2^-(L+2).  x + 2.0 and the scaling are
 *   exact, so each coordinate is ONE rounded IEEE addition; the offset lies in (0, 2^-L], so a point may sit on its
 *   cell's upper edge.  From c = (re, im) on everything is the reference's: cardioid / bulb rejection, IterateMandelbrot,
 *   the accept filter, IterateAndRecord into the histogram, and every cb_counters field with its normal meaning.
 *
 * What the image means: the density of a normal render restricted to the samples of the listed cells -- the normal
 * image minus what the unlisted cells would have contributed (the known bias of an importance map; a longer probe and a
 * larger dilation shrink it).  n_cells / n^2 is the factor between focused and uniform sample counts.
 *
 * Two kernels (draw_focus.hip): CB_KERNEL_DEFAULT, lanes refilled from their own subsequence with the exact-periodicity
 * early-out, and CB_KERNEL_SIMPLE, the definition in lock-step; optionally | CB_KERNEL_FLAG_BURNING_SHIP; any other
 * variant is hipErrorInvalidValue.  Identical masks, histograms, generator states and counters (but skipped_steps).
 * Direct atomics, no workspace, no carry: every launch is complete when it ends. */
#define CB_FOCUS_MIN_LEVEL 4
#define CB_FOCUS_MAX_LEVEL 10
/* Bytes of a mask of this level (n * n / 8; 0 for a level out of range). */
size_t cb_focus_mask_bytes(int level);
/* The probe: ORs into d_mask (cb_focus_mask_bytes(level) of device memory, zeroed by the caller before the first
 * launch), advances d_states like a normal launch, adds to d_counters (may be NULL). */
int cb_focus_probe(const cb_fractal_dimensions *dims, const cb_iteration_control *iterations, void *d_states,
                   uint32_t n_threads, uint32_t samples_per_thread, int level, uint32_t *d_mask,
                   cb_counters *d_counters, int kernel_variant, void *stream);
/* Host side of the cell list, from a mask in HOST memory: *n_cells receives the number of cells of the dilated mask;
 * cells_out (may be NULL: count only) receives them and must hold that many entries (n * n always suffices).
 * hipErrorInvalidValue for a level out of range, dilate < 0 or a NULL mask or n_cells. */
int cb_focus_cells(int level, const uint32_t *mask_host, int dilate, uint32_t *cells_out, uint32_t *n_cells);
/* The focused draw: as cb_draw_buddhabrot without workspace and carry, with the samples drawn from d_cells[0 .. n_cells)
 * (device memory, entries below n * n).  n_cells = 0 is hipErrorInvalidValue.  For tests, d_cells == NULL && n_cells == 0
 * && level == 0 selects the UNIFORM source: a normal render through this kernel, equal to cb_draw_buddhabrot's bit for
 * bit. */
int cb_draw_buddhabrot_focus(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                             const cb_iteration_control *iterations, void *d_states, uint32_t n_threads,
                             uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, int level,
                             const uint32_t *d_cells, uint32_t n_cells, void *stream);

/* ---- Projected render: any 2-D projection of the 4-D Buddhabrot ---------------- *
 *
 * Every recorded orbit point is a point (z_re, z_im, c_re, c_im) of a four-dimensional set; the normal render plots its
 * (z_re, z_im) shadow.  A PROJECTION is eight doubles P[2][4], row-major: rows (u, v), columns in the order (z_re, z_im,
 * c_re, c_im).  Entries must be finite; anything else is hipErrorInvalidValue.
 *
 *   Samples.  The normal stream, four XORWOW draws per sample; the same cardioid / bulb rejection (not for the Burning
 *   Ship), the same IterateMandelbrot, the same accept filter min <= k < max.  The replay visits exactly the points
 *   IterateAndRecord visits: z_1 ... z_{k+1}, the escaping point included.
 *
 *   Plot.  Each visited point z of a sample c is plotted at
 *       K_u = fma(P[0][2], c_re, P[0][3] * c_im)                  (once per sample)
 *       u   = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u))
 *   and v likewise from row 1.  Every operation is IEEE fp64, each fma one rounding, nothing else contracted.  (u, v) is
 *   then binned exactly as the reference bins (re, im), with u in the place of re and v in the place of im: the same
 *   `x < min` early-out, (int) ((x - min) / delta) and bounds tests.  The canvas (w, h, min_real ... max_imag) describes
 *   the (u, v) window.
 *
 *   Counters keep their normal meaning; skipped_steps is the executed-work discount, as in every product kernel.
 *
 *   Identity.  P = {{1,0,0,0},{0,1,0,0}} is a normal render bit for bit: histogram, generator states and every counter
 *   but skipped_steps.  Every visited z is finite -- the point before an escaping one has |z|^2 <= 4, so the escaping
 *   point itself is bounded -- and c is finite, so each zero entry contributes a product that is exactly +0 or -0, never
 *   NaN: K_u = +-0, fma(0, z_im, K_u) = +-0, and u = fma(1, z_re, +-0) = z_re, except that u may be +0 where z_re is -0
 *   (or the reverse).  +0 and -0 compare equal in `x < min`, and x - min differs at most in the sign of a zero, which
 *   (int) (x / delta) maps to pixel 0 either way: a +-0 difference cannot move a bin.
 *
 * Two kernels (draw_plot.hip): CB_KERNEL_DEFAULT, lanes refilled from their own subsequence, with the interior map
 * (Mandelbrot step only) and the exact-periodicity early-out, and CB_KERNEL_SIMPLE, the definition in lock-step;
 * optionally | CB_KERNEL_FLAG_BURNING_SHIP; any other variant, CB_KERNEL_FLAG_ANTI included, is hipErrorInvalidValue.
 * (| CB_KERNEL_POWER(d) instead of the Burning Ship's flag: the Multibrot step and its two kernels, "Multibrot step";
 * | CB_KERNEL_FORMULA(f) instead of either: a formula step and its two kernels, "Formula step".)
 * Identical histograms, generator states and counters (but skipped_steps).  Direct atomics, no workspace, no carry:
 * every launch is complete when it ends.  The -s buffer format is unchanged and does NOT record the plane: resuming a
 * buffer with another projection adds two different images, and nothing can notice. */
int cb_draw_buddhabrot_projected(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                 const cb_iteration_control *iterations, const double projection[8], void *d_states,
                                 uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                 int kernel_variant, void *stream);

/* ---- Julia render: the Buddhabrot of a Julia set on the projected path ------------ *
 *
 * Every other render samples c and starts the orbit at z_0 = c.  A JULIA render fixes c and samples the starting point:
 * it is a projected render ("Projected render" above) with one change to where the sample goes.  The project's own
 * definition (the reference has none).  Normative:
 *
 *   Parameter.  julia_c[2] = (c_re, c_im), both finite and in [-2, 2]; anything else is hipErrorInvalidValue.
 *
 *   Samples.  The normal stream: four XORWOW draws per sample, two coordinates (s_re, s_im) in [-2, 2)^2.  The sample is
 *   z_0.  Nothing is rejected: no cardioid or bulb test and no interior map, so rejected = 0.
 *
 *   Iteration.  z_{n+1} = step(c, z_n) with the fixed c.  The step is the reference's (mandel_step), its Burning Ship
 *   variant under CB_KERNEL_FLAG_BURNING_SHIP, or the Multibrot step of degree d under CB_KERNEL_POWER(d) ("Multibrot
 *   step", not together with the Burning Ship), each the same sequence of IEEE fp64 operations as in the other renders,
 *   bit for bit.
 *
 *   Escape index.  k is the index of the first z_{k+1} with |z|^2 > 4 among z_1 ... z_max; if there is none, k = max and
 *   the sample is never_escaped.  z_0 is neither tested nor plotted, just as the reference neither tests nor plots
 *   z_0 = c.
 *
 *   Accept filter and replay.  min <= k < max; the replay visits z_1 ... z_{k+1}, the escaping point included.
 *
 *   Plot.  The visited point is (z_re, z_im, c_re, c_im) WITH THE FIXED c: K_u and K_v are computed from julia_c, not
 *   from the sample; u, v and the binning are exactly the projected render's.  A plane that uses only c-axes is
 *   degenerate (every point lands on one pixel); it is allowed.
 *
 *   Counters mean what they mean for a Multibrot render; skipped_steps is the executed-work discount of the product
 *   kernel, and the lock-step kernel leaves it 0.
 *
 *   Every visited point is finite: |z_0|^2 <= 8, so |z_1| <= 8^(d/2) + |c| <= 4096 + 2 sqrt 2, and every later visited
 *   point follows a point with |z|^2 <= 4.
 *
 * Two kernels (draw_plot.hip): CB_KERNEL_DEFAULT, one instance per step, lanes refilled from their own subsequence, with
 * the exact-periodicity early-out -- all that retires a Julia interior: attracting cycles land on an exact fp64 cycle
 * quickly -- and CB_KERNEL_SIMPLE, the definition in lock-step with step and degree run-time arguments; optionally
 * | CB_KERNEL_FLAG_BURNING_SHIP or | CB_KERNEL_POWER(d), or | CB_KERNEL_FORMULA(f) instead of either ("Formula step");
 * any other variant, CB_KERNEL_FLAG_ANTI included, is
 * hipErrorInvalidValue, with nothing launched or written.  Identical histograms, generator states and counters (but
 * skipped_steps).  Direct atomics, no workspace, no carry: every launch is complete when it ends.  The -s buffer records
 * c no more than it records the plane or the degree. */
int cb_draw_buddhabrot_julia(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2], void *d_states, uint32_t n_threads,
                             uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant, void *stream);

/* ---- Palette render: orbits coloured by their escape index -------------------------- *
 *
 * A Buddhabrot is usually shown coloured by how long its orbits took to escape.  A PALETTE render is a projected render
 * ("Projected render" above; julia_c NULL) or a Julia render ("Julia render"; julia_c given), and those sections,
 * together with "Multibrot step", apply unchanged: the sample stream, rejection, the interior map where the Mandelbrot
 * step has one, the iteration, the escape index k, the accept filter min <= k < max, the replayed points z_1 ... z_{k+1},
 * the projection's four fused operations and the binning.  What changes is where an in-canvas point goes and with what
 * weight.  The project's own definition (the reference has none).  Normative:
 *
 *   Table.  lut has n_entries uint32_t entries and n_entries == max_escape_iterations, 1 <= n_entries <=
 *   CB_PALETTE_MAX_ENTRIES (2^24).  Entry k carries the weights of an orbit with escape index k: R = bits 0-7, G = bits
 *   8-15, B = bits 16-23.  Bits 24-31 are not read by the kernels.  Entries below min_escape_iterations are never looked
 *   up.
 *
 *   Histogram.  Three planes of w*h cb_pixel, plane 0 = R, 1 = G, 2 = B, contiguous: the layout of a three-channel
 *   histogram.  An in-canvas point of an accepted orbit adds weight_j to its pixel in plane j, for every j with
 *   weight_j != 0.  Integer weights keep the histogram a pure function of the sample stream: hard windows are the table
 *   whose entries are 0 or 1 per plane, the plain render is the constant table 0x010101.
 *
 *   Counters.  samples, rejected, never_escaped, too_fast, recorded, iterate_steps and replay_steps are exactly what the
 *   same render without a palette counts: an accepted orbit whose entry is all zero still counts in recorded and
 *   replay_steps.  increments is the sum of the weights added -- what the histogram gains, as the anti-Buddhabrot counts
 *   it.  skipped_steps is the executed-work discount: the product kernel does not replay an orbit whose entry is zero
 *   and adds its k + 1 replay steps to skipped_steps; the lock-step kernel replays everything and leaves it 0.
 *
 *   Stops -> table (cb_palette_from_stops, host only).  1 to CB_PALETTE_MAX_STOPS (16) stops (k, r, g, b), k >= 0
 *   strictly ascending, components 0 .. 255.  For k <= k_first the entry is the first stop's colour, for k >= k_last the
 *   last stop's.  For adjacent stops a, b with k_a <= k < k_b each component is
 *       (v_a * (k_b - k) + v_b * (k - k_a) + (k_b - k_a) / 2) / (k_b - k_a)
 *   in uint64_t, both divisions truncating.  The entry is r | g << 8 | b << 16.  Anything else is hipErrorInvalidValue.
 *
 *   Image.  Let M be the largest counter of all three planes together.  Each counter maps to cb_tone_value(count, M,
 *   gamma): cb_set_grayscale_pixels applied to the three planes as one w x 3h image.  A common maximum, because the
 *   ratio between a pixel's planes is its colour; no percentile stretch.  The file is the binary PPM of "Colour image"
 *   step 5 below: P6, 65535, big-endian R, G, B per pixel, rows as in the PGM.
 *
 * Two kernels (draw_plot.hip): CB_KERNEL_DEFAULT, one instance per step and per source of c (sampled, fixed), lanes
 * refilled from their own subsequence with the exact-periodicity early-out and, for the Mandelbrot step on a sampled c,
 * the interior map under cb_draw_buddhabrot_projected's rule; CB_KERNEL_SIMPLE, the definition in lock-step.  Variants
 * are cb_draw_buddhabrot_julia's (| CB_KERNEL_FLAG_BURNING_SHIP, | CB_KERNEL_POWER(d) or | CB_KERNEL_FORMULA(f), the last
 * with the two kernels of "Formula step").  Identical histograms,
 * generator states and counters (but skipped_steps).  Direct atomics, no workspace, no carry: every launch is complete
 * when it ends.  The -s buffer has three planes and records the table no more than it records the plane, the degree or
 * c. */
#define CB_PALETTE_MAX_ENTRIES (1 << 24)
#define CB_PALETTE_MAX_STOPS 16
typedef struct {
  int k;       /* escape index of the stop, >= 0 */
  int r, g, b; /* 0 .. 255 */
} cb_palette_stop;
/* The table of the stops (host arithmetic only): lut_out receives n_entries entries.  hipErrorInvalidValue, with lut_out
 * untouched: a NULL pointer, n_stops outside 1 .. CB_PALETTE_MAX_STOPS, n_entries outside 1 .. CB_PALETTE_MAX_ENTRIES, a
 * negative k, stops not strictly ascending in k, a component outside 0 .. 255. */
int cb_palette_from_stops(const cb_palette_stop *stops, int n_stops, uint32_t *lut_out, uint32_t n_entries);
/* The palette draw on caller-owned device memory: d_hist is THREE planes of w*h cb_pixel, d_lut the table on the device.
 * julia_c NULL: c is sampled (a projected render); else the fixed c of a Julia render.  hipErrorInvalidValue, with
 * nothing launched or written: a NULL table, n_entries != iterations->max_escape_iterations, n_entries outside 1 ..
 * CB_PALETTE_MAX_ENTRIES, and everything cb_draw_buddhabrot_projected (julia_c NULL) or cb_draw_buddhabrot_julia
 * refuses. */
int cb_draw_buddhabrot_palette(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2], const uint32_t *d_lut,
                               uint32_t n_entries, void *d_states, uint32_t n_threads, uint32_t samples_per_thread,
                               cb_counters *d_counters, int kernel_variant, void *stream);

/* ---- Depth render: the 4-D set sliced along a third axis into N planes --------------- *
 *
 * A projected render shows the shadow of the four-dimensional set on a plane: it integrates over the two directions that
 * are not plotted.  A DEPTH render keeps one of them: it is a projected render ("Projected render" above; julia_c NULL)
 * or a Julia render ("Julia render"; julia_c given) with one more parameter block, cb_depth below, and those sections,
 * together with "Multibrot step" and "Formula step", apply unchanged: the sample stream, rejection, the interior map
 * where the Mandelbrot step on a sampled c has one, the iteration, the escape index, the accept filter min <= k < max,
 * the replayed points z_1 ... z_{k+1}, (u, v) and their binning.  N = 1 is a SECTION of the set (only the points whose
 * depth lies in the window), N > 1 a VOLUME (the "3-D Buddhabrot" is the (z_re, z_im, c_re) case).  The project's own
 * definition (the reference has none).  Normative:
 *
 *   Parameter.  cb_depth: the depth row D[4], columns in the order (z_re, z_im, c_re, c_im), every entry finite; the
 *   depth window [min, max), both finite, min < max and max - min finite; the number of slices N, 1 <= N <=
 *   CB_DEPTH_MAX_SLICES.  Anything else is hipErrorInvalidValue, and so is N * h > INT_MAX.
 *
 *   Depth of a visited point.
 *       K_d = fma(D[2], c_re, D[3] * c_im)                        (once per sample; for a Julia render once, from the
 *                                                                  fixed c)
 *       d   = fma(D[0], z_re, fma(D[1], z_im, K_d))
 *   -- the same fused operations as u and v: IEEE fp64, each fma one rounding, nothing else contracted.
 *
 *   Slice.  delta_d = (max - min) / (double) N, made on the host exactly as cb_recompute_pixel_deltas makes delta_imag.
 *   The point is IN DEPTH iff !(d < min) and s = (int) ((d - min) / delta_d) satisfies 0 <= s < N: the reference's
 *   binning of `im`, with the same early-out, the same truncation and the same bounds test.  (A kernel may multiply by
 *   the reciprocal where delta_d is a power of two, as the binning of (u, v) does: that is the same value.)
 *
 *   Histogram.  N planes of w*h cb_pixel, contiguous, plane s at offset s*w*h (64-bit arithmetic).  A visited point that
 *   is on the canvas and in depth adds 1 to its pixel of plane s.  Every other point adds nothing.
 *
 *   Counters.  increments counts the points added.  Every other counter is what the same render without a depth counts;
 *   skipped_steps is the product kernel's executed-work discount as usual, and the lock-step kernel leaves it 0.
 *
 *   Consequences.  The sum of the planes is the projected or Julia render restricted to the points in depth; if the
 *   window holds every visited point, that sum is the projected or Julia render itself, bit for bit.  (|z_0|^2 <= 8 and
 *   every later point follows one with |z|^2 <= 4, so every visited |z| of a step of degree d is at most
 *   (2 sqrt 2)^d + 2 sqrt 2: 8 + 2 sqrt 2 for degree 2.)
 *
 *   No table.  A depth render of a palette render -- 3 N planes -- is out of scope and refused.
 *
 *   Image.  Let M be the largest counter of all N planes together.  Each counter maps to cb_tone_value(count, M, gamma):
 *   cb_set_grayscale_pixels applied to the planes as one w x N*h image.  A common maximum, because the ratio between
 *   slices is the volume's density.  The file is N binary PGMs back to back (Netpbm's format allows a sequence of images
 *   in a file), slice 0 first, each "P5\n%d %d\n65535\n" and w*h big-endian u16; with N = 1 an ordinary PGM.
 *
 * Two kernels (draw_depth.hip): CB_KERNEL_DEFAULT, one instance per step and per source of c, lanes refilled from their
 * own subsequence with the exact-periodicity early-out and, for the Mandelbrot step on a sampled c, the interior map
 * under cb_draw_buddhabrot_projected's rule; CB_KERNEL_SIMPLE, the definition in lock-step.  Variants are
 * cb_draw_buddhabrot_julia's: optionally | CB_KERNEL_FLAG_BURNING_SHIP, | CB_KERNEL_POWER(d) or | CB_KERNEL_FORMULA(f);
 * anything else is hipErrorInvalidValue, with nothing launched or written.  Identical histograms, generator states and
 * counters (but skipped_steps).  Direct atomics, no workspace, no carry: every launch is complete when it ends.  The -s
 * buffer has N planes and records the row and the window no more than it records the plane, the degree or c. */
#define CB_DEPTH_MAX_SLICES 256
typedef struct {
  double row[4];   /* the depth row D: columns (z_re, z_im, c_re, c_im), finite */
  double min, max; /* the depth window [min, max), finite, min < max */
  int slices;      /* N, 1 .. CB_DEPTH_MAX_SLICES */
} cb_depth;
/* The depth draw on caller-owned device memory: d_hist is N = depth->slices planes of w*h cb_pixel.  julia_c NULL: c is
 * sampled (a projected render); else the fixed c of a Julia render.  hipErrorInvalidValue, with nothing launched or
 * written: a NULL depth, a non-finite row entry or bound, min >= max, N outside 1 .. CB_DEPTH_MAX_SLICES, N * h > INT_MAX,
 * and everything cb_draw_buddhabrot_projected (julia_c NULL) or cb_draw_buddhabrot_julia refuses. */
int cb_draw_buddhabrot_depth(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2], const cb_depth *depth, void *d_states,
                             uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                             void *stream);

/* ---- Depth-palette render: orbit points coloured by their depth, into three planes --- *
 *
 * The N planes of a depth render are a volume, not a picture, and their memory grows with N.  A DEPTH-PALETTE render
 * decides the colour where the point is plotted: the slice of a visited point indexes a table of N colours, and the point
 * adds that colour's three integer weights to three planes -- the palette render's mechanism keyed by depth instead of
 * escape index.  The histogram is three planes whatever N is, and the image is one PPM: the depth-cued colour render the
 * "3-D Buddhabrot" is known for.  It is a depth render ("Depth render" above) with a table, and that section applies
 * unchanged but for its Histogram, Counters, No table and Image.  The project's own definition.  Normative:
 *
 *   Inputs.  The cb_depth of "Depth render" (row D, window [min, max), N from 1 to CB_DEPTH_MAX_SLICES) and a table lut of
 *   n_entries == N uint32_t entries in the palette's entry format ("Palette render", Table): R = bits 0-7, G = bits 8-15,
 *   B = bits 16-23; bits 24-31 are not read by the kernels.  Entry s carries the weights of a point in slice s.
 *
 *   Unchanged from "Depth render".  The sample stream, rejection, the interior map under cb_draw_buddhabrot_projected's
 *   rule, the iteration, the accept filter, the replayed points, u, v, d, K_d, delta_d, the slice s and its bounds test.
 *
 *   Histogram.  Three planes of w*h cb_pixel, plane 0 = R, 1 = G, 2 = B, contiguous.  A visited point that is on the
 *   canvas and in depth adds weight_j(lut[s]) to its pixel of plane j, for every j with weight_j != 0.  Every other point
 *   adds nothing.
 *
 *   Counters.  increments is the sum of the weights added.  Every other counter is what the depth render counts: the
 *   lock-step kernel leaves skipped_steps 0, the product kernel's is its usual executed-work discount (the entry is known
 *   per point, not per orbit: no orbit is left unreplayed for its colour).
 *
 *   Stops -> table.  cb_palette_from_stops(stops, n, lut, N), unchanged, with k read as a slice index.
 *
 *   Image.  As "Palette render", Image: the three planes tone-mapped against their common maximum, a P6 PPM.
 *
 *   Consequences.  With V the planes of cb_draw_buddhabrot_depth under the same arguments: plane j equals the sum over s
 *   of weight_j(lut[s]) * V[s], bit for bit; a table that is 1 in plane 0 at one slice and 0 elsewhere gives that slice;
 *   the constant table 0x010101 with N = 1 gives the section three times.
 *
 * Two kernels (draw_depth_palette.hip), with the variants, the refusals and the agreement of the depth render's two.  The
 * product kernel keeps the table, at most 1 KiB, in LDS.  A palette render with a depth ("Palette render" by escape index
 * AND N slices, 3 N planes) stays refused.  The -s buffer has three planes and records the table, the row and the window
 * no more than it records the plane, the degree or c. */
/* The depth-palette draw on caller-owned device memory: d_hist is THREE planes of w*h cb_pixel, d_lut the table on the
 * device.  hipErrorInvalidValue, with nothing launched or written: a NULL table, n_entries != depth->slices, and
 * everything cb_draw_buddhabrot_depth refuses. */
int cb_draw_buddhabrot_depth_palette(const cb_fractal_dimensions *dims, cb_pixel *d_hist,
                                     const cb_iteration_control *iterations, const double projection[8],
                                     const double julia_c[2], const cb_depth *depth, const uint32_t *d_lut, uint32_t n_entries,
                                     void *d_states, uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                                     int kernel_variant, void *stream);

/* ---- Frames render: F rotated (or otherwise projected) frames from one orbit pass ---- *
 *
 * The picture the 4-D set is known for is the turn: the Buddhabrot rotating into the bifurcation diagram.  The iteration
 * is the part of a plotted render that does not depend on the plane, so one pass can serve every frame.  A FRAMES render
 * is a projected render ("Projected render" above; julia_c NULL) or a Julia render ("Julia render"; julia_c given) with F
 * matrices instead of one, and those sections, "Multibrot step" and "Formula step" apply unchanged but for the plot, the
 * histogram and one counter.  The project's own definition.  Normative:
 *
 *   Inputs.  n_frames = F, 1 <= F <= CB_FRAMES_MAX; F matrices P_f[2][4], contiguous, 8 doubles each in the order of
 *   "Projected render", every entry finite; F * h <= INT_MAX.  Anything else is hipErrorInvalidValue, with nothing
 *   launched or written.
 *
 *   Unchanged.  The sample stream (four draws per sample), rejection, the interior map under
 *   cb_draw_buddhabrot_projected's rule, the iteration, the escape index, the accept filter min <= k < max, and the
 *   replayed points z_1 .. z_{k+1}.
 *
 *   Plot.  For every visited point and every f:
 *     K_u = fma(P_f[0][2], c_re, P_f[0][3] * c_im)
 *     u   = fma(P_f[0][0], z_re, fma(P_f[0][1], z_im, K_u))
 *   and v likewise from row 1 -- the projected render's four fused operations -- then its binning.  A point on the canvas
 *   of frame f adds 1 to its pixel of plane f.
 *
 *   Histogram.  F planes of w*h cb_pixel, plane f at offset f*w*h (64-bit arithmetic): the depth render's layout.
 *
 *   Counters.  increments counts the points added, over all planes.  Every other counter is what ONE projected or Julia
 *   render with any one of the matrices counts: an accepted orbit counts once in recorded and its k+1 steps once in
 *   replay_steps.  skipped_steps is the product kernel's executed-work discount; the lock-step kernel leaves it 0.
 *
 *   Consequence.  Plane f equals the histogram of cb_draw_buddhabrot_projected (or _julia) with P_f, bit for bit, under the
 *   same dims, iteration control, variant, generators and launch sequence; the generator states and every counter but
 *   increments are equal as well, and the frames render's increments is the sum of the F renders'.  F = 1 is that render
 *   in everything.
 *
 *   Sweep -> matrices.  cb_frames_from_sweep below: frame f is `base` rotated in the (X, Y) coordinate plane by
 *     a_f = deg0 + ((deg1 - deg0) * (double) f) / (double) n_frames
 *   -- three fp64 operations in that order; deg1 is exclusive, so 0:360:F closes a loop -- with the arithmetic of
 *   cb_rotate_projection, which is the `--rotate` flag's.  Every frame is made from `base`, never from the frame before.
 *
 *   Image.  As "Depth render", Image: M is the largest counter of all F planes, each counter maps to cb_tone_value(count,
 *   M, gamma), and the file is F binary PGMs back to back, frame 0 first.  The common maximum is the point: the sequence
 *   has one exposure.
 *
 * Two kernels (draw_frames.hip): CB_KERNEL_DEFAULT, one instance per step and per source of c, lanes refilled from their
 * own subsequence, the visited points queued per wave in LDS and plotted 64 lanes wide; CB_KERNEL_SIMPLE, the definition
 * in lock-step.  Variants and their refusals are cb_draw_buddhabrot_julia's.  Frames of a depth or palette render are out
 * of scope and refused. */
#define CB_FRAMES_MAX 256
/* Rotates both rows of p in the (axis_x, axis_y) coordinate plane by `degrees`: with (a, b) the two entries of a row,
 * a' = (a co - b si) + 0.0 and b' = (a si + b co) + 0.0 (an exact zero is +0).  An integer multiple of 90 degrees uses
 * exact co, si in {0, +-1}; otherwise co = cos(degrees * (M_PI / 180.0)) and si = sin of the same, the host's.  Returns 0;
 * hipErrorInvalidValue with p untouched for a NULL p, equal axes, an axis outside 0 .. 3 or a non-finite angle.  Host only. */
int cb_rotate_projection(double p[8], int axis_x, int axis_y, double degrees);
/* The matrices of a rotation sweep ("Frames render", Sweep -> matrices): out receives n_frames x 8 doubles, angles_out
 * (may be NULL) the n_frames angles a_f.  hipErrorInvalidValue with out and angles_out untouched: a NULL base or out,
 * equal axes or an axis outside 0 .. 3, a non-finite deg0, deg1 or entry of base, n_frames outside 1 .. CB_FRAMES_MAX.
 * Host only. */
int cb_frames_from_sweep(const double base[8], int axis_x, int axis_y, double deg0, double deg1, int n_frames, double *out,
                         double *angles_out);
/* The frames draw on caller-owned device memory: d_hist is F = n_frames planes of w*h cb_pixel, d_frames the F matrices ON
 * THE DEVICE.  julia_c NULL: c is sampled.  The matrices are validated from a host copy: the call copies them back on
 * `stream` and waits for it before it launches.  hipErrorInvalidValue, with nothing launched or written: a NULL d_frames,
 * F outside 1 .. CB_FRAMES_MAX, a non-finite entry, F * h > INT_MAX, a julia_c outside [-2, 2]^2, and any kernel_variant
 * cb_draw_buddhabrot_julia refuses (CB_KERNEL_FLAG_ANTI and CB_KERNEL_FLAG_DRAIN among them). */
int cb_draw_buddhabrot_frames(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                              const double *d_frames, int n_frames, const double julia_c[2], void *d_states,
                              uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                              void *stream);

/* ---- Phoenix render: a step with memory, z^2 + c + p z_prev, on the projected path -------- *
 *
 * Every other step is memoryless: the next point is a function of (z, c).  The PHOENIX recurrence (Ushiki) is
 * z_{n+1} = z_n^2 + c + p z_{n-1}; with real data it is the Henon map (c = -a, p = b).  A Phoenix render is a projected
 * render ("Projected render"; julia_c NULL) or a Julia render ("Julia render"; julia_c given) with that step and one more
 * parameter, p.  The project's own definition (the reference has none).  Normative:
 *
 *   Parameter.  phoenix_p[2] = (p_re, p_im), both finite and in [-2, 2]; anything else is hipErrorInvalidValue.  p = (0, 0)
 *   is allowed.
 *
 *   Samples.  The normal stream: four XORWOW draws per sample, two coordinates (s_re, s_im) in [-2, 2)^2.  Without a fixed c
 *   the sample is c and z_0 = c, as in a projected render; with julia_c the sample is z_0 and c is fixed, exactly as in
 *   "Julia render".  Nothing is rejected, whatever p is: no cardioid or bulb test and no interior map (neither is valid for
 *   p != 0, and one rule is simpler than two), so rejected = 0.
 *
 *   State and step.  The state of an orbit is the pair (z, y), y the point before z, and y_0 = 0.  With z = (r, i), one step
 *   is mandel_step's four operations followed by four fused ones:
 *       ii = i*i;  t = fma(r, r, -ii);  nr = cr + t;  ni = fma(r + r, i, ci);            (mandel_step, bit for bit)
 *       nr = fma(p_re, y_re, nr);  nr = fma(-p_im, y_im, nr);
 *       ni = fma(p_re, y_im, ni);  ni = fma( p_im, y_re, ni);
 *       y = (r, i);  z = (nr, ni);  m = fma(ni, ni, nr*nr)                               (|z|^2 as tested)
 *   -- IEEE fp64, every fma one rounding, nothing else contracted; the negation of p_im is exact.  The iteration and the
 *   replay make the same step, so a replayed orbit retraces the tested one bit for bit.
 *
 *   Escape index.  k is the index of the first z_{k+1} with |z|^2 > 4 among z_1 ... z_max; if there is none, k = max and
 *   the sample is never_escaped.  z_0 is neither tested nor plotted.
 *
 *   Accept filter and replay.  min <= k < max; the replay starts from (z_0, y_0 = 0) and visits z_1 ... z_{k+1}, the
 *   escaping point included.
 *
 *   Plot.  The visited point is (z_re, z_im, c_re, c_im) under P[2][4]: K_u, K_v, u, v and the binning are the projected
 *   render's, from the sample where c is sampled and from julia_c where it is fixed.  y is state, not a plotted
 *   coordinate.
 *
 *   Counters keep their meaning; skipped_steps is the product kernel's executed-work discount, and the lock-step kernel
 *   leaves it 0.
 *
 *   Every visited point is finite: |z_0|^2 <= 8; every later step follows a z with |z|^2 <= 4 and a y that is 0, z_0 or
 *   such a z, so |z| <= 4 + 2 sqrt 2 + 2 sqrt 2 |p| at worst, |p| <= 2 sqrt 2.  Zero entries of P therefore contribute
 *   exact +-0.
 *
 *   Consequences.  fma(+-0, finite, x) = x up to the sign of a zero, which changes neither an escape test nor a bin
 *   ("Identity" above).  So with p = (0, 0) and julia_c = C the Phoenix render equals cb_draw_buddhabrot_julia with the same
 *   C -- histogram, generator states and every counter but skipped_steps --, and with p = (0, 0) and a sampled c it equals
 *   the projected render without its rejection and its interior map.
 *
 * Two kernels (draw_phoenix.hip): CB_KERNEL_DEFAULT, the round scheduler with one instance per source of c, and
 * CB_KERNEL_SIMPLE, the definition in lock-step.  The scheduler's exact-periodicity test compares the whole state (z, y)
 * with the saved one: for a step with memory z_k == z_saved alone proves nothing about z_{k+1}.  The step is the render's
 * own, so ANY flag bit of kernel_variant -- the Burning Ship, anti, a power, a formula, drain -- is hipErrorInvalidValue with
 * nothing launched or written.  Identical histograms, generator states and counters (but skipped_steps).  Direct atomics,
 * no workspace, no carry: every launch is complete when it ends.  Plotting y (a 2 x 6 matrix), and Phoenix with a palette,
 * a depth, frames, a focus, channels or the anti render, are out of scope and refused. */
int cb_draw_buddhabrot_phoenix(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2] /* NULL: sampled c */,
                               const double phoenix_p[2], void *d_states, uint32_t n_threads, uint32_t samples_per_thread,
                               cb_counters *d_counters, int kernel_variant, void *stream);

/* ---- Bounded render: the orbits that never escape, on any plane, under any plotted step -- *
 *
 * CB_KERNEL_FLAG_ANTI plots the orbits that do not escape on (z_re, z_im) under the reference's step or the Burning Ship.
 * A BOUNDED render plots the same orbits on the plane a matrix picks, under any step of the plotted path and with a sampled
 * or a fixed c: the attractor of the 4-D set where the projected render plots its escaping halo.  On the plane (z_re, c_re)
 * it is the bifurcation diagram of the logistic map itself.  The project's own definition (the reference has none).
 * Normative:
 *
 *   Samples and step.  The same sample stream as every render: four XORWOW draws per sample, two coordinates
 *   (s_re, s_im) in [-2, 2)^2, and lane t advances generator t by exactly its samples.  The step S is any step of the
 *   plotted path: the reference's, its Burning Ship variant (CB_KERNEL_FLAG_BURNING_SHIP), z^D + c for D = 3 ... 8
 *   (CB_KERNEL_POWER, "Multibrot step") or one of the five formulas (CB_KERNEL_FORMULA, "Formula step"), each bit for bit
 *   the step of those renders.
 *
 *   Source of c.  julia_c NULL: c is the sample and z_0 = c.  julia_c given: c = julia_c is fixed, both parts in [-2, 2],
 *   and z_0 is the sample, exactly as in "Julia render".
 *
 *   Escape.  With z_k = S(z_{k-1}, c) and M = max_escape_iterations, a sample escapes if |z_k|^2 > 4 for some
 *   1 <= k <= M.  z_0 is neither tested nor plotted.
 *
 *   Nothing is rejected: there is no cardioid or bulb test and no interior map, whatever the step and the source of c; the
 *   launch reports interior-map level 0.  min_escape_iterations is ignored.
 *
 *   An escaping sample adds nothing.  A sample that does not escape adds the M points (z_k, c), k = 1 ... M: each is the
 *   point (z_re, z_im, c_re, c_im) under P[2][4], projected with the four fused operations of "Projected render" in the
 *   same order -- K_u = fma(P[0][2], c_re, P[0][3] * c_im), u = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u)), v likewise
 *   from row 1 -- and (u, v) binned as the projected render bins it, into ONE plane of w*h cb_pixel.
 *
 *   M <= 0.  Nothing is tested and nothing is added, as under CB_KERNEL_FLAG_ANTI.
 *
 *   Counters, exactly as CB_KERNEL_FLAG_ANTI defines them: rejected = 0; never_escaped = recorded = the samples that do not
 *   escape; too_fast = the escaping samples; iterate_steps = sum of k over the escaping samples (k the step that escaped)
 *   + M per sample that does not; replay_steps = M * recorded; increments = what the histogram gains; skipped_steps = the
 *   part of iterate_steps + replay_steps not executed, the only counter the two kernels may differ in.
 *
 *   Consequence.  With the identity matrix and a sampled c, u = z_re and v = z_im up to the sign of a zero ("Identity"
 *   above), so the bounded render under the reference's step or the Burning Ship equals cb_draw_buddhabrot with
 *   CB_KERNEL_FLAG_ANTI: histogram, generator states and every counter but skipped_steps.
 *
 * Two kernels (draw_bounded.hip).  CB_KERNEL_SIMPLE is the definition in lock-step: every point with weight 1.
 * CB_KERNEL_DEFAULT is the product kernel, one instance per step and per source of c, with the anti render's cycle
 * compression: c is constant along an orbit and the plotted point is a function of (z_k, c) only, so if z_n == z_s bit for
 * bit the orbit from z_s on is the cycle z_s ... z_{n-1} repeated and so are its plotted points; the histogram of the
 * transient z_1 ... z_{s-1} once plus ONE period, in which the point z_{s+j} carries the weight floor((M - s - j) / p) + 1,
 * p = n - s, equals the naive one bit for bit (integer adds commute).  Identical histograms, generator states and counters
 * (but skipped_steps).  Direct atomics, no workspace, no carry: every launch is complete when it ends.
 *
 * kernel_variant: what cb_draw_buddhabrot_julia accepts -- CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, optionally with ONE of
 * CB_KERNEL_FLAG_BURNING_SHIP, CB_KERNEL_POWER(D), CB_KERNEL_FORMULA(F).  hipErrorInvalidValue, with nothing launched and
 * the histogram, the counters and the generators untouched: CB_KERNEL_FLAG_ANTI, CB_KERNEL_FLAG_DRAIN, the timed and
 * full-iterate variants and every other base variant, the Burning Ship with a degree, a formula with the Burning Ship or a
 * degree, a degree or a code out of range, a non-finite matrix entry, a julia_c outside [-2, 2]^2 (a NaN included).
 * Bounded orbits under the Phoenix step, into a palette, a depth or frames, with a focus or channels, and on more than one
 * GPU are out of scope. */
int cb_draw_buddhabrot_bounded(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2] /* NULL: sampled c */, void *d_states,
                               uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                               void *stream);

/* ---- Aimed render: a cropped plotted render sampled only from the cells that reach it -- *
 *
 * Every plotted render draws its samples uniformly over [-2, 2)^2, so a crop -- a zoom into the Feigenbaum diagram, one
 * window of a Julia set's orbits -- costs what the full picture costs and is far noisier.  The AIMED render is to the
 * plotted renders what the focused render ("Focused render" above) is to the normal one.  The project's own definition.
 * Normative:
 *
 *   An aimed render is an UN-AIMED render plus a cell list.  The un-aimed render is a projected render ("Projected
 *   render": matrix P, any step of the plotted renders, c sampled or fixed by julia_c) or a bounded render ("Bounded
 *   render"), with one plane and no table.
 *
 *   Sample plane, grid, mask, list.  The sample plane is the plane the stream's samples lie in: with a sampled c that is
 *   c (and z_0 = c); with a fixed c it is z_0.  Grid, level (CB_FOCUS_MIN_LEVEL .. CB_FOCUS_MAX_LEVEL), mask layout,
 *   dilation and the ascending list are exactly the focused render's: cb_focus_mask_bytes and cb_focus_cells serve both.
 *
 *   Probe.  A launch of the un-aimed render on the normal stream (four draws per sample) that adds nothing to a histogram.
 *   A sample marks the cell that holds the SAMPLE when its plotted orbit -- z_1 .. z_{k+1} of an accepted escaping orbit,
 *   z_1 .. z_M of a bounded one -- has at least one point that the binning accepts.  The cell is found as the focused
 *   render finds it: exact scaling, and the value 2.0 clamped into the last cell.  The replay ends at that point.  The mask
 *   is a union of bits, so it does not depend on the schedule.
 *
 *   Probe counters.  Everything up to the replay is counted as the un-aimed render counts it.  recorded is the number of
 *   marking samples; replay_steps the steps made up to and including the first in-canvas point, or all of them where there
 *   is none; increments is 0.  For a bounded orbit replayed cycle-compressed the index of the first in-canvas point is the
 *   naive replay's: the compressed replay visits z_1 .. z_{s-1+p} in the naive order, and any later point is bit for bit
 *   one of those.
 *
 *   Aimed draw.  Each sample takes six generator outputs, mapped exactly as "Focused render" maps them.  From the sample on
 *   everything is the un-aimed render's, with the un-aimed render's counter meanings: cardioid / bulb rejection only for
 *   the Mandelbrot step with a sampled c on the escaping kind; the interior map by the projected render's own rule for
 *   that same case, and never for bounded; the accept filter; the cycle-compressed weights for bounded.
 *
 *   Bias.  As "Focused render": the image is the un-aimed image of the same samples density minus what the unlisted cells
 *   would have added; a cell no probed sample reached from is dark.
 *
 *   Consequences.  With no list (level 0, no cells) the aimed draw is the un-aimed render bit for bit: histogram,
 *   generator states and counters.  With the identity matrix, the reference's step, a sampled c and escaping orbits the
 *   probe's mask is cb_focus_probe's and the draw from a list is cb_draw_buddhabrot_focus's -- histogram, generator states
 *   and counters, skipped_steps apart (the aimed draw consults the interior map, the focused one has none).
 *
 * Kernels (draw_aim.hip).  CB_KERNEL_SIMPLE is the definition in lock-step, every point with weight 1; CB_KERNEL_DEFAULT
 * the product kernels on the round scheduler, the un-aimed render's mode behind the cell source.  The variants are those
 * cb_draw_buddhabrot_julia / cb_draw_buddhabrot_bounded accept.  Aimed renders into a palette, period-palette, depth,
 * depth-palette or frames sink, under the Phoenix step, weighted cells and more than one GPU are out of scope. */

/* The probe: ORs into d_mask (cb_focus_mask_bytes(level) bytes on the device, zeroed by the caller before the first
 * launch) the cells whose samples reach the canvas.  julia_c NULL: c is sampled.  bounded != 0: the bounded kind.
 * hipErrorInvalidValue, nothing written: a NULL pointer but julia_c / d_counters / stream, a canvas without pixels, a matrix
 * that is not finite, a c outside [-2, 2]^2, a level out of range, a variant the un-aimed entry point refuses. */
int cb_aim_probe(const cb_fractal_dimensions *dims, const cb_iteration_control *iterations, const double projection[8],
                 const double julia_c[2] /* NULL: sampled c */, int bounded, void *d_states, uint32_t n_threads,
                 uint32_t samples_per_thread, int level, uint32_t *d_mask, cb_counters *d_counters, int kernel_variant,
                 void *stream);
/* The aimed draw from d_cells[0 .. n_cells) of the level's grid (device memory, ascending, as cb_focus_cells lists them).
 * level 0 with d_cells NULL and n_cells 0 is the uniform source: the un-aimed render through this kernel.
 * hipErrorInvalidValue, nothing written: whatever cb_draw_buddhabrot_julia / _bounded refuse, and any other combination of
 * level, d_cells and n_cells. */
int cb_draw_buddhabrot_aimed(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                             const double projection[8], const double julia_c[2] /* NULL: sampled c */, int bounded,
                             void *d_states, uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters,
                             int kernel_variant, int level, const uint32_t *d_cells, uint32_t n_cells, void *stream);

/* ---- Period-palette render: bounded orbits coloured by their cycle's period ----------- *
 *
 * The bounded render is the one family without colour, for a bounded orbit has no escape index.  Its natural key is the
 * PERIOD of the cycle it falls onto: with it the plane (c_re, c_im) shows every hyperbolic component of the Mandelbrot set
 * in the colour of its period, and the plane (z_re, c_re) the Feigenbaum diagram with every branch in the colour of its
 * period.  The period the product kernel's cycle compression sees is a multiple of its chunk and a period of the fp64 limit
 * cycle, not of the map; even the least bitwise return is the wrong key (a sample spiralling onto an attracting fixed
 * point has a rounding 2-cycle, or none at all, long before it has converged).  The key is a TOLERANT return time from
 * z_M, as period-colouring programs define it.  A PERIOD-PALETTE render is a bounded render ("Bounded render" above) plus
 * a table, and that section applies unchanged -- the sample stream, the step, the source of c, which samples are bounded,
 * the M points z_1 ... z_M of a bounded sample, the projection and the binning, nothing rejected, no interior map,
 * min_escape_iterations not read, M <= 0 tests and adds nothing -- but for its Histogram and Counters.  The project's own
 * definition.  Normative:
 *
 *   Inputs.  A table lut of n_entries uint32_t entries in the palette's entry format ("Palette render", Table): R = bits
 *   0-7, G = bits 8-15, B = bits 16-23; bits 24-31 are not read.  2 <= n_entries <= CB_PERIOD_MAX_ENTRIES (1024); let
 *   J = n_entries - 1.  A tolerance eps, a finite double >= 0.
 *
 *   Period of a bounded sample.  Its orbit is continued past z_M with the same step and the same c, and no escape test is
 *   made.  For j = 1 ... J, in this operation order and in fp64:
 *     dr = re(z_{M+j}) - re(z_M)
 *     di = im(z_{M+j}) - im(z_M)
 *     d2 = fma(dr, dr, di * di)
 *   The period is the least j with d2 <= eps, and 0 if there is none; a NaN compares false.  It is a pure function of the
 *   sample, M, J, eps, the step and c: no schedule enters.  eps = 0 is an exact return, with +0 and -0 alike.
 *
 *   Histogram.  Three planes of w*h cb_pixel, plane 0 = R, 1 = G, 2 = B, contiguous.  Each of the M points of a bounded
 *   sample with period pi adds weight_j(lut[pi]) to its pixel of plane j, for every j with a non-zero weight.  Entry 0 is
 *   the colour of "no period <= J".
 *
 *   Counters.  The bounded render's, with two differences: increments is the sum of the weights added, and skipped_steps
 *   is the product kernel's executed-work discount (the lock-step kernel leaves it 0).  The steps of the period search are
 *   counted nowhere.  A bounded sample whose entry is all zero still counts in recorded and replay_steps; the product
 *   kernel does not replay it, and books the replay it did not make into skipped_steps.
 *
 *   Stops -> table.  cb_palette_from_stops(stops, n, lut, n_entries), unchanged, with k read as a period.
 *
 *   Image.  As "Palette render", Image: the three planes tone-mapped against their common maximum, a P6 PPM.
 *
 *   Consequences.  The constant table 0x010101 makes each plane equal the bounded render's histogram, bit for bit, with
 *   the same generator states and counters but increments, which is three times as large.  With B_pi the render of the
 *   table that is 0x000001 at entry pi and 0 elsewhere, the sum over pi of B_pi's plane 0 is the bounded histogram, and
 *   any table's plane j is the sum over pi of weight_j(lut[pi]) * B_pi.  Under the reference's step with a sampled c,
 *   eps = 0x1p+10 gives every bounded sample the period 1 (|z_M| <= 2 and |z_{M+1}| < 7).
 *
 * Two kernels (draw_periods.hip), with the variants and the refusals of the bounded render's two.  CB_KERNEL_SIMPLE is the
 * definition in lock-step.  CB_KERNEL_DEFAULT is the product kernel: the bounded render's cycle compression with the
 * search as a scheduled pass in front of the replay.  If z_k == z_s bit for bit, with p = k - s and rem = (M - s) mod p,
 * then z_M is the cycle point z_{s+rem} bit for bit and z_{M+j} what the step makes of it, so walking on from z_s gives the
 * probe after rem steps and every z_{M+j} after that; the replay and its weights are the bounded render's.  Identical
 * histograms, generator states and counters (but skipped_steps).  The table is read once per bounded orbit from global
 * memory.  Periods under the Phoenix step, of the anti render, above 1023, and colouring by the multiplier or the internal
 * angle are out of scope. */
#define CB_PERIOD_MAX_ENTRIES 1024
/* The period-palette draw on caller-owned device memory: d_hist is THREE planes of w*h cb_pixel, d_lut the table on the
 * device.  kernel_variant: what cb_draw_buddhabrot_bounded accepts.  hipErrorInvalidValue, with nothing launched or
 * written: a NULL table, n_entries outside 2 .. CB_PERIOD_MAX_ENTRIES, a period_eps that is negative, infinite or a NaN,
 * and everything cb_draw_buddhabrot_bounded refuses.  No interior map is attached. */
int cb_draw_buddhabrot_periods(const cb_fractal_dimensions *dims, cb_pixel *d_hist, const cb_iteration_control *iterations,
                               const double projection[8], const double julia_c[2] /* NULL: sampled c */,
                               const uint32_t *d_lut, uint32_t n_entries, double period_eps, void *d_states,
                               uint32_t n_threads, uint32_t samples_per_thread, cb_counters *d_counters, int kernel_variant,
                               void *stream);

/* ---- Renderer: SetupCUDA + RenderImage + the -s buffer, as an owned object ---------------------- */

typedef struct cb_renderer cb_renderer;

/* SetupCUDA (cudabrot.cu:153-189): selects `device`, allocates and zeroes the histogram, allocates
 * and initialises n_threads generator states for subsequences [first_subsequence, +n_threads). */
int cb_renderer_create(cb_renderer **out, int device, const cb_fractal_dimensions *dims,
                       const cb_iteration_control *iterations, uint64_t seed,
                       uint64_t first_subsequence, uint32_t n_threads);
/* The same for a fused multi-channel render: n_channels (1..CB_MAX_CHANNELS) windows; the histogram is
 * n_channels planes of w*h counters, in read/write_histogram too (n_channels = 0: cb_renderer_create). */
int cb_renderer_create_channels(cb_renderer **out, int device, const cb_fractal_dimensions *dims,
                                const cb_iteration_control *windows, int n_channels, uint64_t seed,
                                uint64_t first_subsequence, uint32_t n_threads);
/* `passes` iterations of the loop body of RenderImage (cudabrot.cu:483-487), fused into as few
 * launches as possible; returns after the device has finished the draw launches (the scatter of the last one
 * may still be running, beside which the next call's first launch starts).  Orbits still in flight are
 * carried to the next call; cb_renderer_finish (called by the read/write functions below) completes
 * them and waits for everything. */
int cb_renderer_render_passes(cb_renderer *r, uint32_t passes, int kernel_variant);
/* Makes this renderer a FOCUSED one ("Focused render" above); before its first pass, once.  Probes probe_passes
 * reference passes (50 samples per thread each) of FRESH generators rocrand_init(seed, first_subsequence + t, 0) in a
 * temporary buffer -- the renderer's own generators are not touched, so the cell list is a pure function of (seed,
 * threads, canvas, iteration control, step, level, probe_passes, dilate) and a resumed run rebuilds the identical list
 * -- dilates the mask by `dilate` cells and keeps the list; every later cb_renderer_render_passes launches focused
 * draws (CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE only, no CB_KERNEL_FLAG_ANTI, the same CB_KERNEL_FLAG_BURNING_SHIP as
 * here: anything else is hipErrorInvalidValue).  kernel_variant: the kernel and the step of the probe.  Returns
 * CB_ERROR_FOCUS_EMPTY when the list is empty (the renderer is then unchanged), hipErrorInvalidValue for a channel
 * renderer, a projected renderer, a renderer that has rendered or is focused already, a level out of range,
 * probe_passes = 0, dilate < 0. */
int cb_renderer_set_focus(cb_renderer *r, int level, uint32_t probe_passes, int dilate, int kernel_variant);
/* The size of a focused renderer's cell list and of its grid (n * n): their quotient is the part of the plane the
 * samples are drawn from.  0 and 0 for a renderer without focus.  Either pointer may be NULL. */
int cb_renderer_focus_cells(const cb_renderer *r, uint32_t *n_cells, uint32_t *n_total);
/* Makes this renderer a PROJECTED one ("Projected render" above); before its first pass, once.  Every later
 * cb_renderer_render_passes launches projected draws (CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE, optionally with the Burning
 * Ship's flag, CB_KERNEL_POWER(d) or CB_KERNEL_FORMULA(f): anything else is hipErrorInvalidValue); render_passes, finish and the histogram, image and state reads
 * work as for a focused renderer.  hipErrorInvalidValue for a channel renderer, a focused renderer, a renderer that has
 * rendered or is projected already, or a non-finite entry; cb_renderer_set_focus on a projected renderer is refused
 * likewise. */
int cb_renderer_set_projection(cb_renderer *r, const double projection[8]);
/* A projected renderer's matrix: returns 1 and fills out[8]; returns 0 and leaves `out` alone for a renderer without
 * one (or a NULL argument). */
int cb_renderer_projection(const cb_renderer *r, double out[8]);
/* Makes this renderer a JULIA one ("Julia render" above); before its first pass, once.  projection: the matrix, NULL for
 * the identity.  Every later cb_renderer_render_passes launches Julia draws (CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE,
 * optionally with the Burning Ship's flag, CB_KERNEL_POWER(d) or CB_KERNEL_FORMULA(f): anything else is
 * hipErrorInvalidValue).
 * hipErrorInvalidValue for a channel renderer, a focused or projected renderer, a renderer that has rendered or is a Julia
 * one already, a non-finite matrix entry, or a c that is not two numbers in [-2, 2].  A Julia renderer is a projected
 * one: cb_renderer_projection returns its matrix, cb_renderer_set_focus and cb_renderer_set_projection are refused. */
int cb_renderer_set_julia(cb_renderer *r, const double projection[8], const double julia_c[2]);
/* A Julia renderer's c: returns 1 and fills out[2]; returns 0 and leaves `out` alone for any other renderer (or a NULL
 * argument). */
int cb_renderer_julia(const cb_renderer *r, double out[2]);
/* Makes this renderer a PALETTE one ("Palette render" above); before its first pass, once, and after
 * cb_renderer_set_projection or cb_renderer_set_julia where one of them is wanted: alone it means the identity
 * projection.  lut_host is the table in HOST memory; it is copied to the device, and the histogram is reallocated and
 * zeroed as three planes.  Every later cb_renderer_render_passes launches palette draws with the variants of the
 * renderer it was (a projected or a Julia one); render_passes, finish, read / write_histogram (three planes),
 * read_counters, the generator states and cb_renderer_grayscale_plane (planes 0 .. 2, each with its own maximum, as for
 * channels) work on the three planes.  hipErrorInvalidValue for a channel or focused renderer, a renderer that has
 * rendered or has a palette already, a NULL table, a table with any bit 24-31 set, n_entries !=
 * max_escape_iterations or outside 1 .. CB_PALETTE_MAX_ENTRIES.  Afterwards cb_renderer_set_projection,
 * cb_renderer_set_julia and cb_renderer_set_focus are refused. */
int cb_renderer_set_palette(cb_renderer *r, const uint32_t *lut_host, uint32_t n_entries);
/* A palette renderer's table: returns 1 and sets *n_entries (may be NULL); returns 0 and leaves it alone for any other
 * renderer (or a NULL renderer). */
int cb_renderer_palette(const cb_renderer *r, uint32_t *n_entries);
/* Gives this renderer a DEPTH ("Depth render" above); on a projected or Julia renderer, before its first pass, once --
 * the order on a renderer is projection, then julia, then depth.  The histogram is reallocated and zeroed as N =
 * depth->slices planes; every later cb_renderer_render_passes launches depth draws with the variants of the renderer it
 * was, and render_passes, finish, read / write_histogram (N planes), read_counters, the generator states and
 * cb_renderer_grayscale_plane (planes 0 .. N - 1, each with its own maximum, as for channels) work on the N planes.
 * hipErrorInvalidValue for a plain, channel, focused or palette renderer, a renderer that has rendered or has a depth
 * already, and whatever "Depth render" refuses of *depth.  Afterwards cb_renderer_set_palette,
 * cb_renderer_set_projection, cb_renderer_set_julia and cb_renderer_set_focus are refused. */
int cb_renderer_set_depth(cb_renderer *r, const cb_depth *depth);
/* A renderer's depth: returns N and fills *out (may be NULL); returns 0 and leaves it alone for a renderer without one
 * (or a NULL renderer). */
int cb_renderer_depth(const cb_renderer *r, cb_depth *out);
/* Gives this renderer a DEPTH PALETTE ("Depth-palette render" above); on a projected or Julia renderer, before its first
 * pass, once.  lut_host is the table in HOST memory, n_entries == depth->slices entries; it is copied to the device, and
 * the histogram is reallocated and zeroed as three planes.  Every later cb_renderer_render_passes launches depth-palette
 * draws with the variants of the renderer it was; render_passes, finish, read / write_histogram (three planes),
 * read_counters, the generator states and cb_renderer_grayscale_plane (planes 0 .. 2) work on the three planes.
 * hipErrorInvalidValue wherever cb_renderer_set_depth is refused, for a renderer that has a depth or a depth palette, a
 * NULL table, a table with any bit 24-31 set, n_entries != depth->slices.  Afterwards cb_renderer_set_depth,
 * cb_renderer_set_palette, cb_renderer_set_projection, cb_renderer_set_julia and cb_renderer_set_focus are refused; the
 * renderer is neither a palette renderer nor one with a depth (cb_renderer_palette and cb_renderer_depth return 0). */
int cb_renderer_set_depth_palette(cb_renderer *r, const cb_depth *depth, const uint32_t *lut_host, uint32_t n_entries);
/* A renderer's depth palette: returns 1, fills *out and sets *n_entries (either may be NULL); returns 0 and leaves them
 * alone for any other renderer (or a NULL renderer). */
int cb_renderer_depth_palette(const cb_renderer *r, cb_depth *out, uint32_t *n_entries);
/* Gives this renderer FRAMES ("Frames render" above); on a projected or Julia renderer, before its first pass, once -- the
 * order on a renderer is projection, then julia, then frames.  frames_host is the n_frames matrices in HOST memory; they
 * are copied to the device, and the histogram is reallocated and zeroed as F = n_frames planes.  The renderer's own
 * projection is no longer plotted.  Every later cb_renderer_render_passes launches frames draws with the variants of the
 * renderer it was; render_passes, finish, read / write_histogram (F planes), read_counters, the generator states and
 * cb_renderer_grayscale_plane (planes 0 .. F - 1, each with its own maximum) work on the F planes.
 * hipErrorInvalidValue for a plain, channel, focused or palette renderer, a renderer with a depth, a depth palette or
 * frames already, a renderer that has rendered, and whatever "Frames render" refuses of the matrices.  Afterwards
 * cb_renderer_set_palette, cb_renderer_set_depth, cb_renderer_set_depth_palette, cb_renderer_set_projection,
 * cb_renderer_set_julia and cb_renderer_set_focus are refused. */
int cb_renderer_set_frames(cb_renderer *r, const double *frames_host, int n_frames);
/* A renderer's frames: returns F and fills out[8 F] (may be NULL); returns 0 and leaves it alone for a renderer without
 * frames (or a NULL renderer). */
int cb_renderer_frames(const cb_renderer *r, double *out);
/* Gives this renderer the PHOENIX step ("Phoenix render" above) with parameter p; on a projected or Julia renderer, before
 * its first pass, once -- the order on a renderer is projection, then julia, then phoenix.  The histogram stays one plane:
 * render_passes, prepare, finish, read / write_histogram, read_counters, the generator states and
 * cb_renderer_grayscale_image work as for a Julia renderer.  Every later cb_renderer_render_passes / cb_renderer_prepare
 * takes CB_KERNEL_DEFAULT or CB_KERNEL_SIMPLE without any flag bit: anything else is hipErrorInvalidValue.
 * hipErrorInvalidValue for a plain, channel, focused or palette renderer, a renderer with a depth, a depth palette, frames
 * or a p already, a renderer that has rendered, and a p that is not two numbers in [-2, 2].  Afterwards
 * cb_renderer_set_palette, cb_renderer_set_depth, cb_renderer_set_depth_palette, cb_renderer_set_frames,
 * cb_renderer_set_projection, cb_renderer_set_julia and cb_renderer_set_focus are refused. */
int cb_renderer_set_phoenix(cb_renderer *r, const double phoenix_p[2]);
/* A Phoenix renderer's p: returns 1 and fills out[2]; returns 0 and leaves `out` alone for any other renderer (or a NULL
 * argument). */
int cb_renderer_phoenix(const cb_renderer *r, double out[2]);
/* Makes this a BOUNDED renderer ("Bounded render" above), before its first pass, once: on a plain renderer it brings the
 * identity projection, as the palette does; a projected or Julia renderer keeps its matrix and its c.  The histogram stays
 * one plane: render_passes, prepare, finish, read / write_histogram, read_counters, the generator states and
 * cb_renderer_grayscale_image work as for a projected renderer, and every later cb_renderer_render_passes launches bounded
 * draws with the variants cb_draw_buddhabrot_bounded accepts.  hipErrorInvalidValue for a channel, focused or palette
 * renderer, a renderer with a depth, a depth palette, frames or the Phoenix step, a bounded renderer, and a renderer that
 * has rendered.  Afterwards every setter -- focus, projection, julia, palette, depth, depth palette, frames, phoenix,
 * bounded -- is refused. */
int cb_renderer_set_bounded(cb_renderer *r);
/* 1 for a bounded renderer, 0 for any other (or a NULL renderer). */
int cb_renderer_bounded(const cb_renderer *r);
/* Makes this a PERIOD-PALETTE renderer ("Period-palette render" above), before its first pass, once, where
 * cb_renderer_set_bounded is admitted: on a plain renderer it brings the identity projection; a projected or Julia renderer
 * without a sink keeps its matrix and its c.  lut_host: n_entries entries on the host, 2 .. CB_PERIOD_MAX_ENTRIES, the top
 * byte of each zero; eps finite and >= 0.  The histogram becomes three planes, as for a palette renderer: read /
 * write_histogram move all three, cb_renderer_period_palette_image makes the picture, and every later
 * cb_renderer_render_passes launches period-palette draws with the variants cb_draw_buddhabrot_bounded accepts.
 * hipErrorInvalidValue, the renderer unchanged: whatever cb_renderer_set_bounded refuses, a NULL table, an entry with a top
 * byte, n_entries out of range, an eps that is negative, infinite or a NaN.  Afterwards every setter is refused. */
int cb_renderer_set_period_palette(cb_renderer *r, const uint32_t *lut_host, uint32_t n_entries, double eps);
/* A period-palette renderer's table length and tolerance: returns 1 and fills what is not NULL; returns 0 and leaves both
 * alone for any other renderer (or a NULL renderer). */
int cb_renderer_period_palette(const cb_renderer *r, uint32_t *n_entries, double *eps);
/* Makes this an AIMED renderer ("Aimed render" above), before its first pass, once.  A plain renderer takes it and gains
 * the identity projection; a projected or Julia renderer without a sink takes it and keeps its matrix and its c; a bounded
 * renderer takes it and stays bounded; nothing else does.  Probes probe_passes passes (>= 1) on fresh generators made from
 * the renderer's seed in temporary buffers, exactly as cb_renderer_set_focus does, dilates the mask by `dilate` (>= 0)
 * cells and keeps the list, so the list is a pure function of (seed, threads, canvas, iterations, matrix, step, c, kind,
 * level, probe passes, dilate) and a resumed run rebuilds it.  kernel_variant names the step (and CB_KERNEL_SIMPLE the
 * lock-step probe); every later cb_renderer_render_passes must carry the same step bits, else hipErrorInvalidValue with
 * nothing launched.  CB_ERROR_AIM_EMPTY when the list is empty (the renderer is then unchanged).  An aimed renderer takes
 * no later setter, cb_renderer_set_aim included. */
int cb_renderer_set_aim(cb_renderer *r, int level, uint32_t probe_passes, int dilate, int kernel_variant);
/* (cells listed, cells of the grid) of an aimed renderer; 0, 0 for any other.  cb_renderer_focus_cells of an aimed renderer
 * stays 0, 0. */
int cb_renderer_aim_cells(const cb_renderer *r, uint32_t *n_cells, uint32_t *n_total);
/* Optional, before the first cb_renderer_render_passes: allocates now what that call would allocate for
 * this kernel variant (the scatter workspaces: tens of GB on a large canvas), so that a caller who times
 * the pass loop -- like the reference's "passes took" line, cudabrot.cu:499-500 -- does not time hipMalloc. */
int cb_renderer_prepare(cb_renderer *r, int kernel_variant);
/* Completes all carried work: afterwards the device histogram and counters account for every sample
 * of every pass rendered so far (needed before using cb_renderer_device_histogram directly). */
int cb_renderer_finish(cb_renderer *r);
/* The cudaMemcpy of cudabrot.cu:496-497: host_out receives w*h cb_pixel. */
int cb_renderer_read_histogram(cb_renderer *r, cb_pixel *host_out);
/* The H2D copy of LoadInProgressBuffer (cudabrot.cu:256-257): REPLACES the device histogram. */
int cb_renderer_write_histogram(cb_renderer *r, const cb_pixel *host_in);
int cb_renderer_read_counters(cb_renderer *r, cb_counters *host_out);
/* True-resume checkpoint: the generator states as an opaque blob of
 * cb_rng_state_bytes(n_threads) bytes.  The reference's -s buffer holds the histogram only, so a
 * resumed run replays seed 1337 from the start (cudabrot.cu:215-258,179); histogram + these states
 * continue the sample stream instead.  Both finish carried work first. */
int cb_renderer_read_rng_states(cb_renderer *r, void *host_out);
int cb_renderer_write_rng_states(cb_renderer *r, const void *host_in);
/* Device pointer of the histogram, for a caller-side RCCL reduce. */
cb_pixel *cb_renderer_device_histogram(cb_renderer *r);
/* The one exchange of the multi-GPU path (the reference has no multi-GPU code): rank r
 * renders with first_subsequence = r * n_threads on its own device, then renderers[0] += renderers[1..n)
 * -- one ncclReduce(ncclUint64, ncclSum, root 0) over xGMI when the renderers sit on n distinct devices
 * (RCCL is loaded on first use), an add kernel when they all share one (rehearsal on a one-GPU box).
 * Finishes carried work of every renderer first. */
int cb_renderers_reduce(cb_renderer *const *renderers, int n);
/* CleanupGlobals (cudabrot.cu:112-119). */
void cb_renderer_destroy(cb_renderer *r);

/* ---- Output stage (host side of the reference) -------------------------------------------------- */

/* SetGrayscalePixels (cudabrot.cu:425-468) on a host histogram: gray_out receives w*h host-endian
 * uint16; *max_out and *scale_out are the two numbers of the "Max value" line (cudabrot.cu:437). */
void cb_set_grayscale_pixels(const cb_pixel *hist, int w, int h, double gamma, uint16_t *gray_out,
                             uint64_t *max_out, double *scale_out);
/* SaveImage (cudabrot.cu:548-577): byte-swaps gray in place and writes the binary PGM.  Returns 0,
 * or 1/2/3 = open / header / pixel-data failure (the reference prints and carries on). */
int cb_save_image(const char *path, uint16_t *gray, int w, int h);

/* The value of one pixel under SetGrayscalePixels: count scaled by 65535/max, gamma-corrected
 * (cudabrot.cu:443-449) or plainly scaled when gamma <= 0 (cudabrot.cu:462-466), as uint16. */
uint16_t cb_tone_value(uint64_t count, uint64_t max, double gamma);
/* SaveImage for pixels that are already big-endian (the output of the device tone map). */
int cb_save_image_be(const char *path, const uint16_t *gray_be, int w, int h);

/* ---- Output stage on the device ---------------------------------------------- */

#define CB_TONE_AUTO 0        /* table when max < 2^24, thresholds above */
#define CB_TONE_LUT 1         /* host-evaluated table over every count in [0, max] */
#define CB_TONE_THRESHOLDS 2  /* host-evaluated smallest count per output value + binary search */

/* SetGrayscalePixels (cudabrot.cu:425-468) + the byte swap of SaveImage (cudabrot.cu:566-570) on a
 * DEVICE histogram: d_gray_be receives w*h big-endian uint16 (the PGM body).  The map itself is
 * evaluated by the host (cb_tone_value) into a table the device looks up, so the bytes equal
 * cb_set_grayscale_pixels + cb_save_image's.  Synchronises `stream`. */
int cb_tone_map_device(const cb_pixel *d_hist, int w, int h, double gamma, int mode,
                       uint16_t *d_gray_be, uint64_t *max_out, double *scale_out, void *stream);
/* The same for a renderer's histogram (finishes carried work first); host_gray_be receives the
 * w*h big-endian pixels: 2 bytes per pixel cross PCIe instead of 8. */
int cb_renderer_grayscale_image(cb_renderer *r, double gamma, int mode, uint16_t *host_gray_be,
                                uint64_t *max_out, double *scale_out);

/* ... for plane `plane` of a multi-channel renderer. */
int cb_renderer_grayscale_plane(cb_renderer *r, int plane, double gamma, int mode, uint16_t *host_gray_be,
                                uint64_t *max_out, double *scale_out);

/* The image of a palette renderer ("Palette render", Image; finishes carried work first): cb_tone_map_device over the
 * three planes as one w x 3h image -- one maximum for all of them -- then one kernel interleaves the planar values.
 * host_rgb_be receives the 3*w*h big-endian u16 of the PPM body (cb_save_ppm_be writes the file); *max_out and
 * *scale_out (may be NULL) the two numbers of the "Max value" line.  hipErrorInvalidValue for a renderer without a
 * palette. */
int cb_renderer_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                              double *scale_out);

/* The image of a renderer with a depth ("Depth render", Image; finishes carried work first): cb_tone_map_device over the
 * N planes as one w x N*h image -- one maximum for all of them.  host_gray_be receives the N*w*h big-endian u16, slice
 * 0 first (the bodies of the N PGMs); *max_out and *scale_out (may be NULL) the two numbers of the "Max value" line.
 * hipErrorInvalidValue for a renderer without a depth. */
int cb_renderer_depth_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_gray_be, uint64_t *max_out,
                            double *scale_out);

/* The image of a renderer with frames ("Frames render", Image): cb_renderer_depth_image's arithmetic and arguments on the
 * F planes, frame 0 first.  hipErrorInvalidValue for a renderer without frames. */
int cb_renderer_frames_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_gray_be, uint64_t *max_out,
                             double *scale_out);

/* The image of a renderer with a depth palette ("Depth-palette render", Image): cb_renderer_palette_image's arithmetic
 * and arguments on its three planes.  hipErrorInvalidValue for a renderer without a depth palette. */
int cb_renderer_depth_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                                    double *scale_out);

/* The image of a period-palette renderer ("Period-palette render", Image): cb_renderer_palette_image's arithmetic and
 * arguments on its three planes, the common maximum over all three.  hipErrorInvalidValue for any other renderer. */
int cb_renderer_period_palette_image(cb_renderer *r, double gamma, int tone_mode, uint16_t *host_rgb_be, uint64_t *max_out,
                                     double *scale_out);

/* ---- White clip: an image exposed against a percentile of its counters ------------- *
 *
 * Every image above is scaled against its LARGEST counter.  Where a few pixels hold counts thousands of times above the
 * rest -- a bounded render onto an attracting cycle -- the rest lands in the lowest output levels.  The white clip picks
 * the white point as an exact order statistic of the u64 counters instead, scales against it and saturates what lies
 * above.  It is the project's own definition (the reference has none).  Normative; host, device and the tests' numpy
 * restatement agree bit for bit:
 *
 *   input: the image's counters as ONE array of n values -- all planes of the image together, exactly the array whose
 *   maximum the unclipped image takes -- and the clip percentage p, a finite double with 0 <= p < 100.
 *     lit     = #{count > 0}.
 *     r       = (uint64_t)((double) lit * (p / 100.0)), clamped to lit - 1 when lit > 0   (cb_white_rank).
 *     white   = the (r + 1)-th largest counter: the largest c with #{count >= c} > r; 0 if lit == 0.
 *     clipped = #{count > white}; by construction clipped <= r.
 *     pixel   = cb_tone_value(min(count, white), white, gamma).  The clamp is on the count, so gamma <= 0, the
 *               reference's unclamped branch, needs no case of its own.
 *   The rank is taken over the lit counters only: a Buddhabrot canvas is mostly zeros, and a rank over all pixels would
 *   make white 0 on any crop.
 *   p = 0 gives white = the maximum and every byte, max and scale of the unclipped functions; p just under 100 gives the
 *   smallest non-zero counter; an all-zero array gives white = 0, scale = inf and a zero image, as unclipped.
 *   Planes that share a maximum unclipped share one white (the three planes of the palette renders, the N planes of a
 *   depth or frames render: the ratios between planes carry the picture); each plane of a channel renderer has its own. */

/* 1 for a valid clip percentage (finite, 0 <= p < 100), else 0. */
int cb_white_clip_ok(double clip_percent);
/* r of the definition for `lit` lit counters; 0 when lit == 0. */
uint64_t cb_white_rank(uint64_t lit, double clip_percent);
/* The definition on a host array of n counters: *white_out, *lit_out, *clipped_out.  0, or hipErrorInvalidValue for a
 * NULL pointer or a bad percentage. */
int cb_white_count(const cb_pixel *hist, uint64_t n, double clip_percent, uint64_t *white_out, uint64_t *lit_out,
                   uint64_t *clipped_out);
/* cb_set_grayscale_pixels with a white clip: gray_out receives w*h host-endian uint16; *max_out (may be NULL) is the true
 * maximum, *scale_out (may be NULL) 65535 / white, the scale applied, *white_out (may be NULL) white.  0, or
 * hipErrorInvalidValue for a NULL hist or gray_out, a canvas without pixels or a bad percentage. */
int cb_set_grayscale_pixels_white(const cb_pixel *hist, int w, int h, double gamma, double clip_percent, uint16_t *gray_out,
                                  uint64_t *max_out, double *scale_out, uint64_t *white_out);
/* cb_white_count on a DEVICE array (8-byte aligned, 1 <= n <= 2^40): a radix select over the u64 counters, one sweep for
 * the maximum and lit, then one 256-bin pass per significant byte of the maximum (none when r = 0); r is made on the
 * host.  The three numbers equal cb_white_count's.  Synchronises `stream`. */
int cb_white_count_device(const cb_pixel *d_hist, uint64_t n, double clip_percent, uint64_t *white_out, uint64_t *lit_out,
                          uint64_t *clipped_out, void *stream);
/* cb_tone_map_device with a white clip: the bytes of cb_set_grayscale_pixels_white + cb_save_image, and its three
 * numbers.  CB_TONE_AUTO chooses by white, not by the maximum, and the table has white + 1 entries: a histogram whose hot
 * pixels pass 2^32 still takes the table when white < 2^24.  At p = 0 the bytes are cb_tone_map_device's. */
int cb_tone_map_device_white(const cb_pixel *d_hist, int w, int h, double gamma, int mode, double clip_percent,
                             uint16_t *d_gray_be, uint64_t *max_out, double *scale_out, uint64_t *white_out, void *stream);
/* A renderer's white clip: an output setting, 0 (the default) = off.  With one set, cb_renderer_grayscale_image and
 * _plane, _palette_image, _depth_palette_image, _period_palette_image, _depth_image and _frames_image use the clipped map
 * over the array they take the maximum of otherwise; *max_out stays the true maximum, *scale_out is 65535 / white.  It may
 * be set and changed at any time: it touches no launch, no histogram and no generator state.  cb_renderer_color_image on
 * a renderer with a clip returns hipErrorInvalidValue with nothing launched (the colour stage has a stretch of its own).
 * hipErrorInvalidValue, the renderer left as it was: a bad percentage. */
int cb_renderer_set_white_clip(cb_renderer *r, double percent);
int cb_renderer_white_clip(const cb_renderer *r, double *percent_out);
/* white, lit and clipped of the last image call made with a clip set; zeros before one, and after every
 * cb_renderer_set_white_clip. */
int cb_renderer_last_white(const cb_renderer *r, uint64_t *white_out, uint64_t *lit_out, uint64_t *clipped_out);

/* ---- Density filter: sparse counters smoothed with a kernel that shrinks as the count grows ---- *
 *
 * A histogram counter of n carries Poisson noise of relative size 1/sqrt(n): the faint regions of an image are salt and
 * pepper.  The density filter (flame renderers' "density estimation") spreads each counter with a binomial kernel whose
 * radius falls as the count rises: a pixel hit once becomes a soft blob, a pixel hit ten thousand times stays a pixel.
 * It runs once per image, on the counters, before the tone map.  It is the project's own definition (the reference has
 * none).  Normative; host, device and the tests' restatement in Python integers agree bit for bit.  All arithmetic on
 * counters is unsigned 64-bit integer; the only floating point is the host's making of the threshold table.
 *
 *   parameters: R, an integer, 1 <= R <= CB_DENSITY_MAX_RADIUS; alpha, a finite double in [1/16, 4] (the CLI's default
 *   0.5); n0, an integer, 1 <= n0 <= 2^20 (default 1).
 *   thresholds (cb_density_thresholds, host only): T[0] = 2^64 - 1, and for r = 1 .. R
 *     T[r] = (uint64_t) floor((double) n0 * pow((double) R / (double) r, 1.0 / alpha)),   in exactly this operation order.
 *   T is non-increasing and T[R] = n0.  Parameters with T[1] >= 2^22 (CB_DENSITY_MAX_SMOOTHED) are refused.
 *   (8, 0.5, 1) gives 64, 16, 7, 4, 2, 1, 1, 1; (4, 0.4, 16) gives 512, 90, 32, 16; (4, 0.5, 9) gives 144, 36, 16, 9.
 *   planes and groups: the input is P planes of h rows of w counters, contiguous; `group` G, 1 or 3, divides P, and planes
 *   jG .. jG + G - 1 are group j.  The KEY of a pixel is the sum of its counters over the G planes of its group (a colour
 *   pixel is smoothed as one thing, so hue does not fringe).  The RADIUS of a pixel with key s >= 1 is the largest r in
 *   0 .. R with r = 0 or s <= T[r]; a pixel with s = 0 adds nothing.
 *   kernel: B_r[i] = C(2r, i + r) for i = -r .. r.  A counter n of a pixel with radius r >= 1 at (y, x) adds
 *     n * B_r[dy] * B_r[dx] * 2^(32 - 4r)
 *   to the accumulator acc of (y + dy, x + dx) of the SAME plane, for every |dy|, |dx| <= r that lies inside the plane;
 *   taps outside the plane are dropped and no plane bleeds into the next.  The weights of one kernel sum to exactly 2^32.
 *   A counter n of a pixel with radius 0 is kept apart: sharp = n at its own place (as if it added n * 2^32 there).
 *   output: out = (sharp << 8) + (acc >> 24): a 64-bit fixed-point count with 8 fraction bits.
 *   No overflow by construction: a smoothed counter is <= T[1] < 2^22, a tap weight <= 2^30, there are at most 289 taps,
 *   so acc < 2^61; an input counter >= 2^55 (CB_DENSITY_MAX_COUNT) is refused with nothing written.  Output and input may
 *   not alias.
 * Consequences: a plane whose every lit key exceeds T[1] comes out as in << 8, bit for bit.  For an input whose lit
 * pixels lie at least R from every border, 0 <= 256 * sum(in) - sum(out) < w * h * P: the unshifted accumulators conserve
 * the mass exactly and only the final floor loses, less than one unit per pixel.  The result depends on no schedule. */
#define CB_DENSITY_MAX_RADIUS 8
#define CB_DENSITY_MAX_SMOOTHED (1ull << 22)
#define CB_DENSITY_MAX_COUNT (1ull << 55)

/* T[0 .. R] of the definition into thresholds_out (R + 1 values).  0, or hipErrorInvalidValue -- nothing written -- for a
 * NULL pointer, an R, alpha or n0 outside its range, or parameters whose T[1] reaches 2^22. */
int cb_density_thresholds(int radius, double alpha, uint64_t n0, uint64_t *thresholds_out);
/* 1 when both filters below accept these arguments (the counters themselves apart): pointers not NULL, w, h, planes > 0,
 * group 1 or 3 dividing planes, 1 <= radius <= 8, a table with T[0] = 2^64 - 1, T[1] < 2^22, non-increasing and
 * T[radius] >= 1, and planes * h * w counters at `out` that do not overlap those at `hist`. */
int cb_density_arguments_ok(const void *hist, int w, int h, int planes, int group, int radius, const uint64_t *thresholds,
                            const void *out);
/* The definition on host arrays, plainly (what --tonemap host calls).  0, or hipErrorInvalidValue with `out` untouched:
 * arguments cb_density_arguments_ok refuses, or a counter >= 2^55. */
int cb_density_filter(const cb_pixel *hist, int w, int h, int planes, int group, int radius, const uint64_t *thresholds,
                      uint64_t *out);
/* cb_density_filter on DEVICE arrays (8-byte aligned, at most 2^40 counters, h <= 16 * 65535, planes <= 65535: the
 * grid's limits, hipErrorInvalidValue beyond them): a maximum pass decides the refusal, then one
 * gather kernel, a workgroup per output tile with the tile and its halo staged in LDS (density.hip).  The values equal
 * cb_density_filter's.  Synchronises `stream`. */
int cb_density_filter_device(const cb_pixel *d_hist, int w, int h, int planes, int group, int radius,
                             const uint64_t *thresholds, uint64_t *d_out, void *stream);
/* A renderer's density filter: an output setting, radius 0 (the default) = off.  With one set, every image call of the
 * white clip's list makes its image from the filtered counters: each plane of a grey, channel, depth or frames renderer
 * on its own (group 1), the three planes of a palette, depth-palette or period-palette renderer as one group of 3.  The
 * filtered array is made for the call and freed after it.  *max_out and *scale_out are those of the filtered array, whose
 * values carry 8 fraction bits; a white clip takes its white point from the filtered values too.  No launch, histogram
 * or generator state knows of it.  cb_renderer_color_image on a renderer with a filter returns hipErrorInvalidValue.
 * hipErrorInvalidValue, the renderer left as it was: parameters cb_density_thresholds refuses (radius 0 apart). */
int cb_renderer_set_density_filter(cb_renderer *r, int radius, double alpha, uint64_t n0);
int cb_renderer_density_filter(const cb_renderer *r, int *radius_out, double *alpha_out, uint64_t *n0_out);

/* ---- Equalised image: an image exposed by the rank of its counters ----------------- *
 *
 * Every image above is one linear-then-gamma curve of the count, and the counters span five to ten decades: no single
 * curve shows the halo and the body at once.  Histogram equalisation maps a pixel to the fraction of the lit pixels that
 * are no brighter, so every output level is used by about as many pixels.  It is the project's own definition (the
 * reference has none).  Normative; host, device and the tests' restatement in Python integers agree bit for bit.  All
 * arithmetic on counters is unsigned 64-bit integer; nothing but cb_tone_value touches floating point.
 *
 *   key: cb_equalize_key(c) keeps the 11 most significant bits of a counter.  For c < 2048, key = c; otherwise
 *     s = floor(log2 c) - 10 and key = (s << 10) + (c >> s).
 *   The key is non-decreasing in c and moves in steps of 0 or 1: key(2047) = 2047, key(2048) = key(2049) = 2048,
 *   key(4095) = 3071, key(4096) = 3072, key(2^63 - 1) = 55295, key(2^64 - 1) = 56319; there are CB_EQUALIZE_KEYS = 56320.
 *   Counts below 2048 are told apart exactly, larger ones to one part in 1024: counters that share a key differ by less
 *   than a thousandth in brightness and get one rank, the ranks between keys stay exact -- and that is what lets ONE sweep
 *   of the counters find the whole curve.
 *   input: the image's counters as ONE array of n values -- all planes of the image together, exactly the array whose
 *   maximum the unflagged image takes -- and gamma.
 *     bins[k]  = #{count > 0 with key(count) = k}; zeros are not counted.
 *     lit      = the sum of bins;  le[k] = the sum of bins[j] over j <= k.
 *     table[0] = 0;  table[k] = cb_tone_value(le[k], lit, gamma) for k >= 1: the rank stands where the count stood and lit
 *                where the maximum stood, so gamma works as before, the gamma <= 0 branch included.  One entry is pinned: for
 *                gamma > 0 the brightest lit key, the one with le[k] = lit, gets 65535.  That is what cb_tone_value(lit, lit,
 *                gamma) is in exact arithmetic; in doubles lit * (65535.0 / lit) rounds below 65535 for about one lit in
 *                seven (162 is one) and the conversion would truncate to 65534.
 *     pixel    = table[key(count)].  When lit = 0 the image is zero.
 * Consequences: the map is monotone in the count; the brightest lit key gets 65535 for gamma > 0; lit counters that are
 * distinct and below 2048 get cb_tone_value(r, lit, gamma), r the rank from 1 for the smallest (the largest, r = lit, by
 * the pinned entry: the same value wherever the doubles give 65535, one level more where they do not); the image of hist << j is the image of hist for every
 * j that overflows no counter (a shift keeps which counters share a key), so the density filter's 8 fraction bits change
 * nothing by themselves.  Planes that share a maximum share one table, as they share one white. */
#define CB_EQUALIZE_KEYS 56320

uint32_t cb_equalize_key(uint64_t count);
/* bins (CB_EQUALIZE_KEYS values), lit and the largest counter of a host array of n counters.  0, or hipErrorInvalidValue
 * with nothing written: a NULL pointer or n = 0. */
int cb_equalize_bins(const cb_pixel *hist, uint64_t n, uint64_t *bins_out, uint64_t *lit_out, uint64_t *max_out);
/* table (CB_EQUALIZE_KEYS values) of the definition from bins and gamma; *keys_out is the number of non-empty bins,
 * *levels_out the number of distinct table values over them.  0, or hipErrorInvalidValue with nothing written: a NULL
 * pointer. */
int cb_equalize_table(const uint64_t *bins, double gamma, uint16_t *table_out, uint64_t *keys_out, uint64_t *levels_out);
/* cb_set_grayscale_pixels, equalised: gray_out receives w*h host-endian uint16; *max_out and *scale_out (may be NULL) are
 * what cb_set_grayscale_pixels reports, the largest counter and 65535 / it; *lit_out (may be NULL) is lit.  0, or
 * hipErrorInvalidValue with nothing written: a NULL hist or gray_out, or a canvas without pixels. */
int cb_set_grayscale_pixels_equalized(const cb_pixel *hist, int w, int h, double gamma, uint16_t *gray_out, uint64_t *max_out,
                                      double *scale_out, uint64_t *lit_out);
/* cb_equalize_bins on a DEVICE array (8-byte aligned, 1 <= n <= 2^40): one streaming sweep (equalize.hip) into
 * bins_out_host, CB_EQUALIZE_KEYS values on the HOST.  The numbers equal cb_equalize_bins'.  hipErrorInvalidValue with
 * nothing written: a NULL pointer, an address that is not 8-byte aligned, n = 0 or n > 2^40.  Synchronises `stream`. */
int cb_equalize_bins_device(const cb_pixel *d_hist, uint64_t n, uint64_t *bins_out_host, uint64_t *lit_out, uint64_t *max_out,
                            void *stream);
/* cb_tone_map_device, equalised: the bytes of cb_set_grayscale_pixels_equalized + cb_save_image into d_gray_be, and its
 * numbers; *keys_out and *levels_out are cb_equalize_table's.  Every output number may be NULL.  The bins come from one
 * sweep, the host makes the table and uploads it, a second kernel looks every pixel up.  Synchronises `stream`. */
int cb_tone_map_device_equalized(const cb_pixel *d_hist, int w, int h, double gamma, uint16_t *d_gray_be, uint64_t *max_out,
                                 double *scale_out, uint64_t *lit_out, uint64_t *keys_out, uint64_t *levels_out, void *stream);
/* A renderer's equalisation: an output setting like the white clip, 0 (the default) = off.  With it on, every image call
 * of the white clip's list makes the equalised image over the array it takes the maximum of otherwise -- the filtered one
 * where a density filter is set; tone_mode is validated and otherwise not read (there is one form); *max_out and *scale_out
 * stay what the unflagged call returns.  No launch, histogram or generator state knows of it.  cb_renderer_color_image on
 * an equalised renderer returns hipErrorInvalidValue.  hipErrorInvalidValue, the renderer left as it was: equalisation
 * turned on on a renderer with a white clip -- and cb_renderer_set_white_clip with a clip above 0 on an equalised one. */
int cb_renderer_set_equalize(cb_renderer *r, int on);
int cb_renderer_equalize(const cb_renderer *r);
/* lit, keys and levels of the last image call made equalised; zeros before one, and after every cb_renderer_set_equalize. */
int cb_renderer_last_equalize(const cb_renderer *r, uint64_t *lit_out, uint64_t *keys_out, uint64_t *levels_out);

/* ---- Locally equalised image: one rank curve per tile of the canvas, blended between tile centres -- *
 *
 * The equalised image above is still ONE curve for the whole canvas, and a Buddhabrot is not one population: the filaments
 * beside the body share the bottom few percent of the global ranks.  Contrast-limited adaptive equalisation gives every
 * tile of the canvas a rank curve of its own, interpolates the curves between the tile centres and limits with a clip how
 * far a tile may amplify its contrast.  The project's own definition (the reference has none).  Normative; host, device
 * and the tests' restatement in Python integers agree bit for bit.  All arithmetic on counters, ranks and weights is
 * unsigned 64-bit integer; cb_tone_value (inside cb_equalize_table) stays the only floating point.
 *
 *   input: the image's counters, `planes` planes of h rows of w counters -- the array whose maximum the unflagged image
 *     takes, seen as planes --; a tile grid TX x TY with 1 <= TX, TY <= CB_LOCAL_EQUALIZE_MAX_TILES, TX <= w, TY <= h; a
 *     clip clip_q in 1/256ths, 0 (off) or 256 .. 65536; gamma.
 *   tiles: ex[i] = floor(i * w / TX) for i = 0 .. TX, ey[j] likewise from h and TY.  Tile (i, j), number t = j * TX + i, is
 *     columns [ex[i], ex[i+1]) and rows [ey[j], ey[j+1]) of EVERY plane: planes that share a maximum share one table per
 *     tile, as they share one table equalised -- which keeps the hue of the three palette renders and the ratio between
 *     the slices of a depth or frames render.  A channel plane is an image of its own (planes = 1).
 *   bins: bins_t[k] = the number of lit counters of tile t with cb_equalize_key(count) = k; lit_t their sum, keys_t the
 *     number of non-empty bins; bins_all the sum over the tiles and lit its sum.
 *   clip: with clip_q = 0, clipped_t = bins_t.  Else L_t = max(1, floor(clip_q * lit_t / (256 * keys_t))) (the product is
 *     below 2^57), E_t = the sum over k of max(0, bins_t[k] - L_t), and for the m-th lit key k in ascending order (m from 0)
 *       clipped_t[k] = min(bins_t[k], L_t) + floor(E_t / keys_t) + (m < E_t mod keys_t ? 1 : 0).
 *     Empty bins stay empty, so the sum of clipped_t is lit_t, and every lit key keeps at least 1, so the table stays
 *     strictly increasing in rank over the lit keys.  One redistribution pass, no iteration.  The excess goes to the tile's
 *     LIT keys only -- the project's choice, not the textbook's: the 56 320 keys are almost all empty in any tile.
 *   tables: table_t = cb_equalize_table(clipped_t, gamma).  A tile with lit_t = 0 takes cb_equalize_table(bins_all, gamma),
 *     the global curve, unclipped: an empty tile beside a lit one then pulls its neighbours towards the global image and
 *     not towards black (the corners of the default canvas lie outside radius 2).
 *   pixel (x, y) of any plane, counter c, k = key(c).  Tile centres are kept doubled, so they are integers:
 *     CX[i] = ex[i] + ex[i+1], px = 2x + 1; CY[j] and py likewise.  The columns: if TX = 1 or px <= CX[0],
 *     (i0, i1, ax, dx) = (0, 0, 0, 1); if px >= CX[TX-1], (TX-1, TX-1, 0, 1); otherwise i0 is the largest i with
 *     CX[i] <= px, i1 = i0 + 1, ax = px - CX[i0], dx = CX[i1] - CX[i0].  The rows likewise.  With v_ab = table_(ia, jb)[k]:
 *       num   = (dy - ay) * ((dx - ax) * v00 + ax * v10) + ay * ((dx - ax) * v01 + ax * v11)
 *       pixel = floor((num + floor(dx * dy / 2)) / (dx * dy))
 *     dx * dy <= w * h <= 2^40, so everything stays below 2^57.  A counter of 0 gives 0: every table has table[0] = 0.
 * Consequences: TX = TY = 1 with the clip off is cb_set_grayscale_pixels_equalized bit for bit; at a fixed position the
 * value is monotone in the count; where all lit tiles have equal bins the image is each tile's own equalised image; a pixel
 * with px = CX[i] and py = CY[j] takes table (i, j) alone; the image of hist << s is the image of hist for every s that
 * overflows no counter, so the density filter's 8 fraction bits change nothing by themselves.
 * Reported: lit; lit_tiles, the tiles with lit_t > 0; moved, the sum of E_t over the tiles. */
#define CB_LOCAL_EQUALIZE_MAX_TILES 16

/* 1 if the grid and the clip are ones the definition admits on a canvas of w x h with `planes` planes, else 0. */
int cb_local_equalize_ok(int w, int h, int planes, int tx, int ty, uint32_t clip_q);
/* bins_t of a host array: tx * ty rows of CB_EQUALIZE_KEYS values, tile t = j * tx + i at bins_out + t * CB_EQUALIZE_KEYS;
 * *lit_out is lit, *max_out the largest counter.  0, or hipErrorInvalidValue with nothing written: a NULL pointer or
 * what cb_local_equalize_ok refuses. */
int cb_local_equalize_bins(const cb_pixel *hist, int w, int h, int planes, int tx, int ty, uint64_t *bins_out,
                           uint64_t *lit_out, uint64_t *max_out);
/* clipped_t (CB_EQUALIZE_KEYS values) and E_t of one tile's bins; clipped_out may be bins itself.  0, or
 * hipErrorInvalidValue with nothing written: a NULL pointer, a clip_q that is neither 0 nor in 256 .. 65536. */
int cb_local_equalize_clip(const uint64_t *bins, uint32_t clip_q, uint64_t *clipped_out, uint64_t *moved_out);
/* cb_set_grayscale_pixels, locally equalised: gray_out receives planes*h*w host-endian uint16; *max_out and *scale_out
 * (may be NULL) are what cb_set_grayscale_pixels reports over the whole array; *lit_out, *lit_tiles_out and *moved_out
 * (may be NULL) are the three reported numbers.  0, or hipErrorInvalidValue with nothing written: a NULL hist or gray_out
 * or what cb_local_equalize_ok refuses -- an empty canvas, planes < 1, a grid outside 1 .. 16 or larger than the canvas,
 * a clip_q that is neither 0 nor in 256 .. 65536. */
int cb_set_grayscale_pixels_local_equalized(const cb_pixel *hist, int w, int h, int planes, int tx, int ty, uint32_t clip_q,
                                            double gamma, uint16_t *gray_out, uint64_t *max_out, double *scale_out,
                                            uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out);
/* cb_local_equalize_bins on a DEVICE array (8-byte aligned, planes*h*w <= 2^40): the largest counter first, then one sweep
 * of the tiles (equalize_local.hip) into bins_out_host, tx * ty * CB_EQUALIZE_KEYS values on the HOST.  The numbers equal
 * cb_local_equalize_bins'.  hipErrorInvalidValue with nothing written and nothing read: what the host function refuses, an
 * address that is not 8-byte aligned, more than 2^40 counters, and a canvas whose widest tile row times `planes` is 2^32
 * or more (a block's 32-bit bins could not hold the counters it reads).  Synchronises `stream`. */
int cb_local_equalize_bins_device(const cb_pixel *d_hist, int w, int h, int planes, int tx, int ty, uint64_t *bins_out_host,
                                  uint64_t *lit_out, uint64_t *max_out, void *stream);
/* cb_tone_map_device, locally equalised: the bytes of cb_set_grayscale_pixels_local_equalized + cb_save_image into
 * d_gray_be (planes*h*w big-endian u16), and its numbers; every output number may be NULL.  The bins come from one sweep
 * sized by the largest counter's key, the host clips, makes the tables and uploads them, a second kernel blends four
 * table values per pixel.  Refuses what cb_local_equalize_bins_device refuses and a d_gray_be that is not 4-byte aligned
 * (two pixels are stored at once), with nothing written.  Synchronises `stream`. */
int cb_tone_map_device_local_equalized(const cb_pixel *d_hist, int w, int h, int planes, int tx, int ty, uint32_t clip_q,
                                       double gamma, uint16_t *d_gray_be, uint64_t *max_out, double *scale_out,
                                       uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out, void *stream);
/* A renderer's local equalisation: an output setting like cb_renderer_set_equalize, tx = 0 (the default) = off.  With it
 * on, every image call of the white clip's list makes the locally equalised image over the array it takes the maximum of
 * otherwise -- the filtered one where a density filter is set --, the planes of that image pooled; tone_mode is validated
 * and otherwise not read; *max_out and *scale_out stay what the unflagged call returns.  No launch, histogram, state file
 * or generator state knows of it.  cb_renderer_color_image on such a renderer returns hipErrorInvalidValue.
 * hipErrorInvalidValue, the renderer left as it was: a grid or clip cb_local_equalize_ok refuses on the renderer's canvas
 * (tx = 0 apart), a renderer that is equalised or has a white clip -- and cb_renderer_set_equalize(on) or a clip above 0
 * on a locally equalised one. */
int cb_renderer_set_local_equalize(cb_renderer *r, int tx, int ty, uint32_t clip_q);
int cb_renderer_local_equalize(const cb_renderer *r, int *tx_out, int *ty_out, uint32_t *clip_q_out);
/* lit, lit_tiles and moved of the last image call made locally equalised; zeros before one, and after every
 * cb_renderer_set_local_equalize. */
int cb_renderer_last_local_equalize(const cb_renderer *r, uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out);

/* ---- Colour image: three planes composed into one 16-bit RGB image ------------------------------- *
 *
 * The reference's colour recipe (generate_hires_color_image.sh) renders three windows, stretches each PGM with
 * ImageMagick's `convert -normalize` and merges them with an external HSL combiner.  This stage does the stretch and
 * the merge on the tone-mapped planes.  It is the project's own definition: it is not the external combiner bit for
 * bit (that program is not part of this project).  Normative; host, device and the tests' numpy restatement agree
 * byte for byte (only IEEE + - * floor and compares on the device, no division, no contraction):
 *
 *   input of plane j: v, the 16-bit tone value of each pixel (what the plane's PGM holds; cb_tone_value with the
 *   run's gamma); N = w*h.
 *   1. levels, per plane, with percentages B = black_percent and W = white_percent (ImageMagick's -normalize: 2, 1):
 *        nb = (uint64_t)((double)N * (B / 100.0)),  nw = (uint64_t)((double)N * (W / 100.0));
 *        black = the smallest k with #{v <= k} > nb,  white = the largest k with #{v >= k} > nw.
 *      Valid only for finite B, W with 0 <= B, 0 <= W, B + W < 100.
 *   2. stretch (fp64): s = 0 if v <= black; else s = 1 if v >= white; else s = (double)(v - black) * inv with
 *      inv = 1.0 / (double)(white - black) evaluated by the host (this also covers white <= black).
 *   3. CB_COMPOSE_RGB: out_j = (uint16_t)floor(s_j * 65535.0 + 0.5)  (plane 0 -> R, 1 -> G, 2 -> B).
 *   4. CB_COMPOSE_HSL (fp64, in this order): h = s0 + hue_shift; h = h - floor(h); S = s1; L = s2;
 *        q = L < 0.5 ? L * (1.0 + S) : (L + S) - L * S;  p = 2.0 * L - q;
 *        f(t): t = t - floor(t); t < 1.0/6.0 -> p + ((q - p) * 6.0) * t; t < 0.5 -> q;
 *              t < 2.0/3.0 -> p + ((q - p) * 6.0) * (2.0/3.0 - t); else p;
 *        R = f(h + 1.0/3.0), G = f(h), B = f(h - 1.0/3.0); each clamped to [0, 1], then floor(c * 65535.0 + 0.5).
 *   5. file: binary PPM, header "P6\n%d %d\n65535\n", then w*h pixels of big-endian R, G, B u16, row 0 = the PGMs'. */
#define CB_COMPOSE_RGB 0
#define CB_COMPOSE_HSL 1
typedef struct {
  int compose;           /* CB_COMPOSE_RGB or CB_COMPOSE_HSL */
  double black_percent;  /* B of step 1 */
  double white_percent;  /* W of step 1 */
  double hue_shift;      /* added to the hue (CB_COMPOSE_HSL only); finite */
} cb_color_params;

/* The whole definition on the host: gray[j] are host-endian w*h planes (what cb_set_grayscale_pixels makes);
 * rgb_be receives 3*w*h big-endian u16 (the PPM body); levels (may be NULL) receives black0, white0, black1, ...
 * hipErrorInvalidValue for bad params (compose, percentages, hue shift, sizes) or a NULL pointer. */
int cb_compose_color(const uint16_t *const gray[3], int w, int h, const cb_color_params *p, uint16_t *rgb_be,
                     uint16_t levels[6]);
/* The same from three DEVICE histograms (any cb_pixel planes of w*h): each is tone-mapped with cb_tone_map_device
 * (gamma, tone_mode), the levels are found on the device (two 256-bin radix passes) and one kernel writes the
 * big-endian RGB body to d_rgb_be (3*w*h u16).  Synchronises `stream`; the bytes equal cb_compose_color's on the
 * grays of cb_set_grayscale_pixels. */
int cb_compose_color_device(const cb_pixel *const d_hist[3], int w, int h, double gamma, int tone_mode,
                            const cb_color_params *p, uint16_t *d_rgb_be, uint16_t levels[6], void *stream);
/* For a renderer: finishes carried work, composes planes[0..2] (indices of its channel planes; 0 for a renderer
 * without channels) and copies the 3*w*h big-endian u16 of the RGB body to host_rgb_be. */
int cb_renderer_color_image(cb_renderer *r, const int planes[3], double gamma, int tone_mode,
                            const cb_color_params *p, uint16_t *host_rgb_be, uint16_t levels[6]);
/* Writes the binary PPM of step 5 from a big-endian body; 0, or 1/2/3 = open / header / pixel-data failure (as
 * cb_save_image). */
int cb_save_ppm_be(const char *path, const uint16_t *rgb_be, int w, int h);

const char *cb_error_string(int code);
int cb_abi_version(void);

/* Diagnostics.  The library's test and tuning knobs are environment variables named CUDABROT_AMD_* (DESIGN.md
 * section 7 lists them; none is needed in normal use, all are result-neutral).  They are read through this one
 * gate: the value of `name`, or NULL unless CUDABROT_AMD_DEBUG=1 is set too -- a stray variable in a user's
 * environment cannot change the path the product takes.  (The reference has no such knobs.) */
const char *cb_debug_knob(const char *name);
/* Where the scatter keeps its arrays in a workspace ("Diagnostics and test knobs"): the carve that
 * cb_draw_buddhabrot[_channels] and cb_flush_scatter[_channels] make of (d_workspace, workspace_bytes) for this canvas
 * and n_threads -- a pure function of the arguments, so a test can write a stream of its own into a workspace and have
 * the flush sort it.  n_channels = 0: the one-plane layout of cb_draw_buddhabrot / cb_flush_scatter (word = row << 16 |
 * col); 1..CB_MAX_CHANNELS: the layout of the _channels entry points.  Host arithmetic only: no device memory is
 * touched and nothing is launched, so it works without a GPU on any non-null d_workspace.  enabled = 0 (everything
 * behind the word format 0): such a workspace is not used, the draw call adds with direct atomics.
 * An array the layout does not have reports offset 0, bytes 0. */
typedef struct cb_scatter_array {
  uint64_t offset; /* bytes from d_workspace */
  uint64_t bytes;  /* as carved (the next array starts on the next 256-byte boundary) */
} cb_scatter_array;
typedef struct cb_scatter_layout {
  uint32_t enabled, n_waves, cap, n_tiles, tiles_x, tiles_y, n_planes, two_level, n_groups, chunked, chunks_per_wave,
      max_regions;
  /* a stream word: col = word & e_col_mask, row = (word >> e_row_shift) & e_row_mask,
   * plane = (word >> e_chan_shift) & e_chan_mask */
  uint32_t e_row_shift, e_col_mask, e_row_mask, e_chan_shift, e_chan_mask;
  uint32_t reserved;
  cb_scatter_array wave_count, stream, a_count, a_base, grouped, region_start, region_count, region_group, owner_first,
      group_first, group_regions, n_regions, chunk_desc, chunk_list, run_start, slice_base, sorted;
} cb_scatter_layout;
/* 0, or hipErrorInvalidValue for a NULL dims / out, a canvas without pixels or n_channels outside 0..CB_MAX_CHANNELS. */
int cb_debug_scatter_layout(const cb_fractal_dimensions *dims, int n_channels, uint32_t n_threads,
                            const void *d_workspace, size_t workspace_bytes, cb_scatter_layout *out);
/* Which draw kernel the last cb_draw_buddhabrot* call of this process launched (the renderer's calls included):
 * 0 none yet, 1 draw_wave_kernel (four waves per SIMD), 2 draw_wide_kernel (two waves per SIMD, runs beside the
 * scatter), 3 the lock-step baseline, 4 the anti product kernel (draw_anti_kernel), 5 the anti lock-step kernel, 6 the
 * focus product kernel (draw_focus_kernel: cb_focus_probe and cb_draw_buddhabrot_focus), 7 the focus lock-step kernel,
 * 8 the projection product kernel (draw_plot_kernel: cb_draw_buddhabrot_projected), 9 the projection lock-step kernel,
 * 10 the Multibrot product kernel (draw_plot_kernel, the projected render's with the power step:
 * cb_draw_buddhabrot_projected with CB_KERNEL_POWER), 11 the Multibrot lock-step kernel, 12 the Julia product kernel
 * (draw_plot_kernel: cb_draw_buddhabrot_julia), 13 the Julia lock-step kernel, 14 the palette product kernel
 * (draw_plot_kernel: cb_draw_buddhabrot_palette), 15 the palette lock-step kernel, 16 the formula product kernel
 * (draw_plot_kernel: the three plotted draws with CB_KERNEL_FORMULA), 17 the formula lock-step kernel, 18 the depth
 * product kernel (draw_depth_kernel: cb_draw_buddhabrot_depth, whatever its step), 19 the depth lock-step kernel, 20 the
 * depth-palette product kernel (draw_depth_palette_kernel: cb_draw_buddhabrot_depth_palette, whatever its step), 21 the
 * depth-palette lock-step kernel, 22 the frames product kernel (draw_frames_kernel: cb_draw_buddhabrot_frames, whatever
 * its step), 23 the frames lock-step kernel, 24 the Phoenix product kernel (draw_phoenix_kernel:
 * cb_draw_buddhabrot_phoenix), 25 the Phoenix lock-step kernel, 26 the bounded product kernel (draw_bounded_kernel:
 * cb_draw_buddhabrot_bounded, whatever its step), 27 the bounded lock-step kernel, 28 the period-palette product kernel
 * (draw_periods_kernel: cb_draw_buddhabrot_periods, whatever its step), 29 the period-palette lock-step kernel, 30 the
 * aim product kernels (draw_aim_kernel: cb_draw_buddhabrot_aimed, and draw_aim_probe_kernel: cb_aim_probe, whatever their
 * step), 31 the aim lock-step kernel.
 * The kernels give identical results; tests use this to know what they covered. */
int cb_debug_last_draw_kernel(void);
/* The level of the interior map the last cb_draw_buddhabrot call of this process used (cells of side 2^-level of the
 * c-plane whose samples provably never escape: the draw kernel retires them without iterating; made and proven by
 * tools/interior_map.c, embedded in the library), 0 if it used none.  Results do not depend on it. */
int cb_debug_interior_map_level(void);
/* The same for ONE renderer's last launch (with several ranks in a process the process-wide figure above is whichever
 * rank's launch came last; the map itself is copied to every device once per process, on its first launch there). */
int cb_renderer_interior_map_level(const cb_renderer *r);

#ifdef __cplusplus
}
#endif
#endif
