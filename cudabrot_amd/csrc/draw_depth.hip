// draw_depth.hip -- the depth render (include/cudabrot_amd.h, "Depth render"): a projected render or a
// Julia render (draw_plot.hip) whose visited points are also projected on a third row D of the 4-D set (z_re, z_im, c_re,
// c_im) and binned along it into N planes:
//   K_d = fma(D[2], c_re, D[3] * c_im)             (once per sample; once per launch for a fixed c)
//   d   = fma(D[0], z_re, fma(D[1], z_im, K_d))
//   in depth iff !(d < min) and s = (int) ((d - min) / delta_d) has 0 <= s < N
// -- the four fused operations of u and v and the reference's binning of `im`.  A point that is on the canvas and in depth
// adds 1 to its pixel of plane s (planes plane_pixels counters apart); every other point adds nothing.  Sample stream,
// rejection, interior map, iteration, escape index, accept filter, replayed points, (u, v) and their binning are the
// projected render's (a sampled c) or the Julia render's (a fixed one), unchanged, and so is every counter but
// increments, which counts the points added.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_depth_simple_kernel        the definition verbatim, one lane per reference thread in lock-step, no early-out;
//                                   step, degree, formula and Julia-or-not are run-time arguments.  Validation baseline (19).
//   draw_depth_kernel<Step, kJulia> the product kernel (18): the round scheduler of draw_rounds.h with DepthMode, which
//                                   wraps PlotMode / JuliaMode of draw_plot.h as PaletteMode does: step, NEXT (with the
//                                   interior map under PlotMode's own rule) and the never-escaping case are theirs, ESCAPED
//                                   also makes K_d of a sampled c, and a replayed point finds its pixel and its slice and
//                                   makes one add.  One instance per step (13) and per source of c (2): 26.
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_depth.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// The lock-step kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_depth_simple_kernel(DepthArgs da) {
  const PlotArgs &pa = da.p;
  const DrawArgs &a = pa.d;
  const int f = pa.formula;
  const int deg = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pa.julia != 0;
  const bool rejects = !julia && f == 0 && deg == 2 && !ship;  // the Mandelbrot step on a sampled c: cardioid and bulb
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
          if (depth_step(f, deg, ship, c_re, c_im, r, i) > 4.0) {
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
      const DepthKernelArgs now = fresh_depth_args();
      const double ku = project_constant(now->p.p[2], now->p.p[3], c_re, c_im);
      const double kv = project_constant(now->p.p[6], now->p.p[7], c_re, c_im);
      const double kd = project_constant(now->row[2], now->row[3], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = depth_step(f, deg, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        const double d = project_point(now->row[0], now->row[1], r, i, kd);
        int row, col, s;
        if (pixel_of(u, v, cv, row, col) && slice_of(d, now->min, now->delta, now->inv_delta, now->pow2, now->slices, s)) {
          add_to_pixel(a.hist + (unsigned long long) s * now->plane_pixels, cv, row, col, 1ull);
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

// ------------------------------------------------------------------------------------------------
// draw_depth_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with DepthMode (draw_depth.h).  The body stands in the kernel, not in a function the
// kernel calls.

template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_depth_kernel(DepthArgs da) {
  const PlotArgs &pa = da.p;
  if constexpr (kJulia) {
    const double ku = project_constant(pa.p[2], pa.p[3], pa.c[0], pa.c[1]);
    const double kv = project_constant(pa.p[6], pa.p[7], pa.c[0], pa.c[1]);
    const double kd = project_constant(da.row[2], da.row[3], pa.c[0], pa.c[1]);
    DepthMode<Step, true> mode{{{pa, make_canvas(pa.d), ku, kv}, pa.c[0], pa.c[1]}, da, kd};
    run_rounds(pa.d, mode);
  } else {
    DepthMode<Step, false> mode{{{pa, make_canvas(pa.d)}}, da};
    run_rounds(pa.d, mode);
  }
}

namespace {

typedef void (*DepthKernel)(DepthArgs);

// The product kernels of one step, [fixed c], and every one there is, by step (draw_plot.h, plot_step_index).
struct StepKernels {
  DepthKernel by[2];
};
#define CB_ROW(Step) {{draw_depth_kernel<Step, false>, draw_depth_kernel<Step, true>}},
constexpr StepKernels kDepthKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kDepthKernels) / sizeof(kDepthKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_depth(const DepthArgs &da, bool lockstep, hipStream_t stream) {
  const PlotArgs &a = da.p;
  if (!depth_launch_ok(da)) return hipErrorInvalidValue;
  if (a.palette != 0 || a.lut != nullptr) return hipErrorInvalidValue;  // no table: 3 N planes are out of scope
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  DepthKernel kernel = nullptr;
  if (lockstep) {
    kernel = draw_depth_simple_kernel;
  } else {
    kernel = kDepthKernels[plot_step_index(a)].by[a.julia != 0];
  }
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, da);
  return hipGetLastError();
}

}  // namespace cb
