// draw_plot.hip -- the plotted renders: every recorded orbit point is a point (z_re, z_im,
// c_re, c_im) of a four-dimensional set, and a 2 x 4 matrix P picks the plane it is plotted on:
//   K_u = fma(P[0][2], c_re, P[0][3] * c_im)             (once per sample; once per launch for a fixed c)
//   u   = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u))
// and v likewise from row 1; (u, v) is binned as the reference bins (re, im).  One launch (PlotArgs, kernels.h) has a
// step, a source of c and a sink.
//
// The projected render (include/cudabrot_amd.h, "Projected render").  Samples, cardioid / bulb rejection
// (not for the Burning Ship), IterateMandelbrot, the accept filter min <= k < max and the replayed points z_1 .. z_{k+1}
// are the normal render's.
//
// The Multibrot Buddhabrot ("Multibrot step") is that render with another step: PlotArgs::degree 2 is the
// reference's step, 3 <= degree <= 8 is z <- z^degree + c, the power made of degree - 1 multiplications by z
// (device_math.h), without cardioid or bulb rejection and without the interior map.
//
// The Julia render ("Julia render"): the Buddhabrot of a Julia set.  c is fixed (PlotArgs::c, julia != 0),
// the sample of the normal stream is the starting point z_0, and the escaping orbits of z <- step(c, z) are plotted as a
// projected render plots them, the point (z_re, z_im, c_re, c_im) with the fixed c.  The step is the reference's, its
// Burning Ship variant or the Multibrot step of degree 3 .. 8.  Nothing is rejected: no cardioid, no bulb, no interior
// map.  z_0 is neither tested nor plotted; k is the index of the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max, the
// accept filter min <= k < max, the replay z_1 .. z_{k+1}.
//
// The palette render ("Palette render"): a projected render or a Julia render whose accepted orbits are
// coloured by their escape index k.  lut[k] carries three integer weights, R in bits 0-7, G in bits 8-15, B in bits
// 16-23, and every in-canvas point of the orbit adds weight_j to its pixel in plane j of a histogram of three planes
// (plane_pixels apart), for every j with a non-zero weight.  Sample stream, rejection, interior map, iteration, escape
// index, accept filter, replayed points, projection and binning are the projected render's (a sampled c) or the Julia
// render's (a fixed one), unchanged.
//
// The formula render ("Formula step"): a projected render, a Julia render or a palette render of either
// whose step is another member of the quadratic family -- tricorn, Celtic, buffalo, perpendicular, Celtic tricorn --
// which differs from the reference's step by a sign or an absolute value in nr or ni (device_math.h, formula_step).
// Everything else is those renders', unchanged; like the Multibrot step a formula has no cardioid or bulb rejection and
// no interior map.
//
// Kernels (the number: cb_debug_last_draw_kernel, which names the entry point and the step, capi.hip)
//   draw_project_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; the
//                               step is a run-time switch.  Validation baseline (9).
//   draw_power_simple_kernel    the lock-step kernel of the Multibrot step (11): the degree is a run-time argument and
//                               the step a run-time loop (power_step).
//   draw_julia_simple_kernel    the lock-step kernel of a fixed c (13); step and degree are run-time arguments.
//   draw_palette_simple_kernel  the lock-step kernel of the table (15); step, degree and Julia-or-not are run-time
//                               arguments.
//   draw_formula_simple_kernel  the lock-step kernel of a formula (17); code, Julia-or-not and table-or-not are run-time
//                               arguments.
//   draw_plot_kernel<Step, kJulia, kPalette>
//                               the product kernel (8 projected, 10 Multibrot, 12 Julia, 14 palette, 16 formula): the
//                               round scheduler of draw_rounds.h with PlotMode, JuliaMode or PaletteMode of draw_plot.h,
//                               one instance per step (the reference's, the Burning Ship, degrees 3 .. 8, five
//                               formulas), per source of c and per sink: 13 x 2 x 2 = 52.  Lanes are refilled from
//                               their own subsequence every kRound steps, a new sample is looked up in the interior
//                               map (Mandelbrot step on a sampled c only) and a marked one retired without iterating,
//                               and an orbit found exactly periodic at a chunk boundary is retired as
//                               never-escaping -- all a Julia interior has: attracting cycles land on an exact fp64
//                               cycle quickly.  With a table, an accepted orbit whose entry is zero adds nothing
//                               anywhere, so it is not replayed: its steps go to skipped_steps.  Same histogram,
//                               generator states and counters as the lock-step kernels (but skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

namespace {

// One step with c = (c_re, c_im); degree 2 is the reference's step or its Burning Ship variant, else the Multibrot step.
__device__ __forceinline__ double plot_step(int degree, bool ship, double c_re, double c_im, double &r, double &i) {
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

// The kernel's arguments read afresh, as draw_common.h's fresh_args reads a DrawArgs: what an accepted orbit alone needs
// (the table, c's columns of the matrix) is loaded where it is used and holds no scalar register across the loops.
typedef const PlotArgs __attribute__((address_space(4))) *PlotKernelArgs;
__device__ __forceinline__ PlotKernelArgs fresh_plot_args() {
  PlotKernelArgs p = (PlotKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The five lock-step kernels: the definition, verbatim, written out in each
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_project_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);
      const double imag = sample_coordinate(rng);
      st.samples++;
      if (!a.burning_ship && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      const int k = escape_index(real, imag, a.max_iter, a.burning_ship);
      if (k >= a.max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) (a.max_iter > 0 ? a.max_iter : 0);
        continue;
      }
      st.iterate_steps += (unsigned long long) k + 1ull;
      if (k < a.min_iter) {
        st.too_fast++;
        continue;
      }
      st.recorded++;
      const double ku = project_constant(pa.p[2], pa.p[3], real, imag);
      const double kv = project_constant(pa.p[6], pa.p[7], real, imag);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          add_to_pixel(a.hist, cv, row, col, 1ull);
          st.increments++;
        }
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// The same with the Multibrot step: nothing is rejected, and the degree is a run-time argument.
__global__ void __launch_bounds__(256) draw_power_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const int d = pa.degree;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);
      const double imag = sample_coordinate(rng);
      st.samples++;
      int k = a.max_iter;  // IterateMandelbrot: the first z_{k+1} that escapes
      {
        double r = real, i = imag;
        for (int it = 0; it < a.max_iter; ++it) {
          if (power_step(d, real, imag, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      if (k >= a.max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) (a.max_iter > 0 ? a.max_iter : 0);
        continue;
      }
      st.iterate_steps += (unsigned long long) k + 1ull;
      if (k < a.min_iter) {
        st.too_fast++;
        continue;
      }
      st.recorded++;
      const double ku = project_constant(pa.p[2], pa.p[3], real, imag);
      const double kv = project_constant(pa.p[6], pa.p[7], real, imag);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = power_step(d, real, imag, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          add_to_pixel(a.hist, cv, row, col, 1ull);
          st.increments++;
        }
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// A fixed c: the sample is z_0, nothing is rejected, and step and degree are run-time arguments.
__global__ void __launch_bounds__(256) draw_julia_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const double c_re = pa.c[0], c_im = pa.c[1];
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const double ku = project_constant(pa.p[2], pa.p[3], c_re, c_im);  // from the fixed c: the same for every sample
  const double kv = project_constant(pa.p[6], pa.p[7], c_re, c_im);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);  // z_0
      const double imag = sample_coordinate(rng);
      st.samples++;
      int k = a.max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < a.max_iter; ++it) {
          if (plot_step(d, ship, c_re, c_im, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      if (k >= a.max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) (a.max_iter > 0 ? a.max_iter : 0);
        continue;
      }
      st.iterate_steps += (unsigned long long) k + 1ull;
      if (k < a.min_iter) {
        st.too_fast++;
        continue;
      }
      st.recorded++;
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = plot_step(d, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          add_to_pixel(a.hist, cv, row, col, 1ull);
          st.increments++;
        }
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// The table: either source of c, and every in-canvas point adds the entry's weights to three planes.
__global__ void __launch_bounds__(256) draw_palette_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pa.julia != 0;
  const bool rejects = !julia && d == 2 && !ship;  // the Mandelbrot step on a sampled c: cardioid and bulb
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);  // z_0, and c too unless c is fixed
      const double imag = sample_coordinate(rng);
      const double c_re = julia ? pa.c[0] : real;
      const double c_im = julia ? pa.c[1] : imag;
      st.samples++;
      if (rejects && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      int k = a.max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < a.max_iter; ++it) {
          if (plot_step(d, ship, c_re, c_im, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      if (k >= a.max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) (a.max_iter > 0 ? a.max_iter : 0);
        continue;
      }
      st.iterate_steps += (unsigned long long) k + 1ull;
      if (k < a.min_iter) {
        st.too_fast++;
        continue;
      }
      st.recorded++;
      const PlotKernelArgs now = fresh_plot_args();
      const uint32_t entry = now->lut[k];  // min_iter <= k < max_iter == n_entries, and 0 <= k
      const double ku = project_constant(now->p[2], now->p[3], c_re, c_im);
      const double kv = project_constant(now->p[6], now->p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = plot_step(d, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          unsigned long long *plane = a.hist;  // of weight j
          for (int j = 0; j < 3; ++j, plane += pa.plane_pixels) {
            const unsigned long long weight = palette_weight(entry, j);
            if (weight != 0ull) {
              add_to_pixel(plane, cv, row, col, weight);
              st.increments += weight;
            }
          }
        }
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// A formula: either source of c and either sink, nothing rejected, and the code is a run-time argument.
__global__ void __launch_bounds__(256) draw_formula_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const int f = pa.formula;
  const bool julia = pa.julia != 0;
  const bool table = pa.palette != 0;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);  // z_0, and c too unless c is fixed
      const double imag = sample_coordinate(rng);
      const double c_re = julia ? pa.c[0] : real;
      const double c_im = julia ? pa.c[1] : imag;
      st.samples++;
      int k = a.max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < a.max_iter; ++it) {
          if (formula_step(f, c_re, c_im, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      if (k >= a.max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) (a.max_iter > 0 ? a.max_iter : 0);
        continue;
      }
      st.iterate_steps += (unsigned long long) k + 1ull;
      if (k < a.min_iter) {
        st.too_fast++;
        continue;
      }
      st.recorded++;
      const PlotKernelArgs now = fresh_plot_args();
      // with a table: min_iter <= k < max_iter == n_entries, and 0 <= k; without one: weight 1 in the one plane there is
      const uint32_t entry = table ? now->lut[k] : 1u;
      const double ku = project_constant(now->p[2], now->p[3], c_re, c_im);
      const double kv = project_constant(now->p[6], now->p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = formula_step(f, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          unsigned long long *plane = a.hist;  // of weight j
          for (int j = 0; j < 3; ++j, plane += pa.plane_pixels) {
            const unsigned long long weight = palette_weight(entry, j);
            if (weight != 0ull) {
              add_to_pixel(plane, cv, row, col, weight);
              st.increments += weight;
            }
          }
        }
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_plot_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with one of the three modes of draw_plot.h.  Step says two things: the step, and
// whether it is the Mandelbrot step -- only then, and only with a sampled c, does NEXT reject cardioid and bulb and look
// the sample up in the interior map, a marked one retired without iterating; every other step iterates whatever is drawn.
// (A short run of tested steps inside NEXT, for the 91 % of uniform samples that escape within four, was built and
// measured: slower)  An escape goes through the accept filter to REPLAY of z_1 .. z_n, each point
// projected and binned (device-scope atomics); an exact cycle never escapes and is counted as the reference counts it,
// the steps not made in skipped_steps.  The early-out's proof uses only that the step is a function of z,
// which z^d + c and every formula are for a given c.
//
// A sampled c (PlotMode): NEXT draws c, z_0 = c, and ESCAPED makes the plot's constant from it.  A fixed c (JuliaMode):
// NEXT draws the sample into the lane's (cr, ci), where the scheduler starts z and restarts it for REPLAY: z_0 = sample.
// The step takes the kernel's c, wave-uniform, instead of the lane's pair, and the plot's constant is made from it once,
// before the first round.  A table (PaletteMode) is either of those with another ESCAPED and another plot: step, NEXT and
// the never-escaping case are theirs.  ESCAPED counts the orbit as they do and then loads its entry, once: the lane keeps
// it through the replay.  A zero entry ends the sample there -- counted as recorded and in replay_steps like any accepted
// orbit, the replay not made in skipped_steps.  A replayed point finds its pixel once and adds each non-zero weight to
// that pixel of its plane.
//
// The body stands in the kernel, not in a function the kernel calls.

template <class Step, bool kJulia, bool kPalette>
__global__ void __launch_bounds__(256) draw_plot_kernel(PlotArgs pa) {
  if constexpr (kPalette && kJulia) {
    const double ku = project_constant(pa.p[2], pa.p[3], pa.c[0], pa.c[1]);
    const double kv = project_constant(pa.p[6], pa.p[7], pa.c[0], pa.c[1]);
    PaletteMode<Step, true> mode{{{pa, make_canvas(pa.d), ku, kv}, pa.c[0], pa.c[1]}, pa.lut, pa.plane_pixels};
    run_rounds(pa.d, mode);
  } else if constexpr (kPalette) {
    PaletteMode<Step, false> mode{{{pa, make_canvas(pa.d)}}, pa.lut, pa.plane_pixels};
    run_rounds(pa.d, mode);
  } else if constexpr (kJulia) {
    JuliaMode<Step> mode{{pa, make_canvas(pa.d)}, pa.c[0], pa.c[1]};
    mode.plot.constant(pa.c[0], pa.c[1]);
    run_rounds(pa.d, mode);
  } else {
    PlotMode<Step> mode{{pa, make_canvas(pa.d)}};
    run_rounds(pa.d, mode);
  }
}

namespace {

typedef void (*PlotKernel)(PlotArgs);

// The product kernels of one step, [fixed c][table], and every one there is, by step (draw_plot.h, plot_step_index).
struct StepKernels {
  PlotKernel by[2][2];
};
#define CB_ROW(Step)                                                                    \
  {{{draw_plot_kernel<Step, false, false>, draw_plot_kernel<Step, false, true>},        \
    {draw_plot_kernel<Step, true, false>, draw_plot_kernel<Step, true, true>}}},
constexpr StepKernels kPlotKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kPlotKernels) / sizeof(kPlotKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_plot(const PlotArgs &a, bool lockstep, hipStream_t stream) {
  const bool julia = a.julia != 0;
  const bool palette = a.palette != 0;
  if (!plot_launch_ok(a)) return hipErrorInvalidValue;
  // every accepted k indexes the table: the table covers [0, max_iter)
  if (palette && (a.lut == nullptr || a.d.max_iter < 1 || a.d.max_iter > CB_PALETTE_MAX_ENTRIES)) {
    return hipErrorInvalidValue;
  }
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  PlotKernel kernel = nullptr;
  if (lockstep) {
    kernel = a.formula != 0  ? draw_formula_simple_kernel
             : palette       ? draw_palette_simple_kernel
             : julia         ? draw_julia_simple_kernel
             : a.degree != 2 ? draw_power_simple_kernel
                             : draw_project_simple_kernel;
  } else {
    kernel = kPlotKernels[plot_step_index(a)].by[julia][palette];
  }
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
