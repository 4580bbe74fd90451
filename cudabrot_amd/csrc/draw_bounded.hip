// draw_bounded.hip -- the bounded render (include/cudabrot_amd.h, "Bounded render"): the orbits of the
// samples that do NOT escape, z_1 .. z_M, each point (z_re, z_im, c_re, c_im) plotted on the plane a 2 x 4 matrix P picks
// and binned as the projected render bins.  It is the anti-Buddhabrot's rule (draw_anti.hip) for which orbits are plotted
// and with what weight, and the plotted renders' (draw_plot.h) for the step, the source of c and where a point goes:
//   the step          the reference's, its Burning Ship variant, z^D + c for D = 3 .. 8, or one of the five formulas;
//   the source of c   sampled (c is the sample, z_0 = c) or fixed (PlotArgs::julia: c = PlotArgs::c, z_0 is the sample);
//   the sink          one u64 plane.
// Nothing is rejected (no cardioid, no bulb, no interior map) and min_iter is not read.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_bounded_simple_kernel     the definition verbatim, one lane per reference thread in lock-step: iterate to M, then
//                                  replay all M points with weight 1.  Step, degree / formula and the source of c are
//                                  run-time arguments.  Validation baseline (27).
//   draw_bounded_kernel<Step, kJulia>
//                                  the product kernel (26): the round scheduler of draw_rounds.h with BoundedMode, one
//                                  instance per step and per source of c: 13 x 2 = 26.  Same histogram, generator states and
//                                  counters (but skipped_steps) with cycle compression: an orbit whose z is bit for bit a
//                                  point it held at an earlier chunk boundary is replayed as its transient plus ONE period,
//                                  each cycle point with its exact integer weight.  c is constant along an orbit and the
//                                  plotted point a function of (z_k, c) only, so equal z are equal plotted points and
//                                  DESIGN.md 4.9's proof carries over (4.21).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// draw_bounded_simple_kernel: the definition, verbatim, written out
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_bounded_simple_kernel(PlotArgs pa) {
  const DrawArgs &a = pa.d;
  const int f = pa.formula;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pa.julia != 0;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter > 0 ? a.max_iter : 0;
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);  // z_0, and c too unless c is fixed
      const double imag = sample_coordinate(rng);
      const double c_re = julia ? pa.c[0] : real;
      const double c_im = julia ? pa.c[1] : imag;
      st.samples++;
      int k = max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < max_iter; ++it) {
          if (bounded_step(f, d, ship, c_re, c_im, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      if (k < max_iter) {  // escaped at z_{k+1}: nothing recorded
        st.too_fast++;
        st.iterate_steps += (unsigned long long) k + 1ull;
        continue;
      }
      st.never_escaped++;
      st.recorded++;
      st.iterate_steps += (unsigned long long) max_iter;
      const double ku = project_constant(pa.p[2], pa.p[3], c_re, c_im);
      const double kv = project_constant(pa.p[6], pa.p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it < max_iter; ++it) {
        (void) bounded_step(f, d, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          add_to_pixel(a.hist, cv, row, col, 1ull);
          st.increments++;
        }
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_bounded_kernel: cycle-compressed, lanes refilled from their own subsequence
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode: no sample is rejected, an escaping one records nothing, and a
// sample that does not escape is replayed -- draw_anti.hip's AntiMode with the plotted renders' step and plot.
//   cycle z_s .. z_{k-1} found (s = saved >= kChunk > 0, k <= M, p = k - s): REPLAY of z_j for j = 1 .. s - 1 + p: z_j,
//            j < s, weight 1; the cycle point z_{s+t}, 0 <= t < p, weight floor((M - s - t) / p) + 1 = q + 1 for t <= rem,
//            q above, with M - s = q p + rem.  Weights sum to (s - 1) + (M - s + 1) = M.
//   k == M without a match: REPLAY of all M points with weight 1.
// A sampled c: NEXT draws c, z_0 = c, and the plot's constant is made from it when the sample is known not to escape.  A
// fixed c: NEXT draws z_0 into the lane's (cr, ci), where the scheduler starts z and restarts it for REPLAY; the step takes
// the kernel's c, wave-uniform, and the plot's constant is made from it once, before the first round.

// The body stands in the kernel, not in a function the kernel calls.
template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_bounded_kernel(PlotArgs pa) {
  BoundedMode<Step, kJulia> mode{{pa, make_canvas(pa.d)}, pa.c[0], pa.c[1]};
  if constexpr (kJulia) mode.plot.constant(pa.c[0], pa.c[1]);
  run_rounds(pa.d, mode);
}

namespace {

typedef void (*BoundedKernel)(PlotArgs);

// The product kernels of one step, [fixed c], and every one there is, by step (draw_plot.h, plot_step_index).
struct BoundedStepKernels {
  BoundedKernel by[2];
};
#define CB_ROW(Step) {{draw_bounded_kernel<Step, false>, draw_bounded_kernel<Step, true>}},
constexpr BoundedStepKernels kBoundedKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kBoundedKernels) / sizeof(kBoundedKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_bounded(const PlotArgs &a, bool lockstep, hipStream_t stream) {
  if (!plot_launch_ok(a) || a.palette != 0 || a.lut != nullptr) return hipErrorInvalidValue;
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const BoundedKernel kernel = lockstep ? draw_bounded_simple_kernel : kBoundedKernels[plot_step_index(a)].by[a.julia != 0];
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
