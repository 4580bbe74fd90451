// draw_julia.hip -- the Julia render (include/cudabrot_amd.h, "Julia render"): the Buddhabrot of a Julia
// set.  c is fixed (JuliaArgs::c), the sample of the normal stream is the starting point z_0, and the escaping orbits of
// z <- step(c, z) are plotted as a projected render plots them, the point (z_re, z_im, c_re, c_im) with the fixed c:
//   K_u = fma(P[0][2], c_re, P[0][3] * c_im)             (once per launch)
//   u   = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u))
// and v likewise from row 1.  The step is the reference's, its Burning Ship variant or the Multibrot step of degree
// 3 .. 8 (device_math.h).  Nothing is rejected: no cardioid, no bulb, no interior map.  z_0 is neither tested nor
// plotted; k is the index of the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max, the accept filter min <= k < max, the
// replay z_1 .. z_{k+1}.
//
// Kernels
//   draw_julia_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; step and
//                             degree are run-time arguments.  Validation baseline (cb_debug_last_draw_kernel 13).
//   draw_julia_kernel<Step>   the product kernel (12), a template over the step: the round scheduler of draw_rounds.h
//                             with the Julia plot mode.  An orbit found exactly periodic at a chunk boundary
//                              is retired as never-escaping -- all a Julia interior has: attracting cycles
//                             land on an exact fp64 cycle quickly.  Same histogram, generator states and counters (but
//                             skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// draw_julia_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

namespace {

// One step with the fixed c; degree 2 is the reference's step or its Burning Ship variant, else the Multibrot step.
__device__ __forceinline__ double julia_step(int degree, bool ship, double c_re, double c_im, double &r, double &i) {
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

}  // namespace

__global__ void __launch_bounds__(256) draw_julia_simple_kernel(JuliaArgs ja) {
  const ProjectArgs &pa = ja.pa;
  const DrawArgs &a = pa.d;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const double c_re = ja.c[0], c_im = ja.c[1];
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
          if (julia_step(d, ship, c_re, c_im, r, i) > 4.0) {
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
        const double m = julia_step(d, ship, c_re, c_im, r, i);
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

// ------------------------------------------------------------------------------------------------
// draw_julia_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode.  NEXT draws the sample into the lane's (cr, ci), where the
// scheduler starts z and restarts it for REPLAY: z_0 = sample.  The step takes the kernel's c, wave-uniform, instead of
// the lane's pair, and the plot's constant is made from it once, before the first round.  The early-out's proof uses only
// that the step is a function of z, which it is for a fixed c.

template <class Step>
__global__ void __launch_bounds__(256) draw_julia_kernel(JuliaArgs ja) {
  JuliaMode<Step> mode{{ja.pa, make_canvas(ja.pa.d)}, ja.c[0], ja.c[1]};
  mode.plot.constant(ja.c[0], ja.c[1]);
  run_rounds(ja.pa.d, mode);
}

hipError_t launch_draw_julia(const JuliaArgs &a, bool lockstep, hipStream_t stream) {
  const ProjectArgs &pa = a.pa;
  const bool power = pa.degree != 2;
  if (power && (pa.degree < CB_POWER_MIN || pa.degree > CB_POWER_MAX || pa.d.burning_ship)) return hipErrorInvalidValue;
  for (int j = 0; j < 2; ++j) {
    if (!(a.c[j] >= -2.0 && a.c[j] <= 2.0)) return hipErrorInvalidValue;  // a NaN fails both comparisons
  }
  if (pa.d.n_threads == 0 || pa.d.samples_per_thread == 0) return hipSuccess;
  void (*kernel)(JuliaArgs) = nullptr;
  if (lockstep) {
    kernel = draw_julia_simple_kernel;
  } else {
    switch (pa.degree) {
      case 2:
        kernel = pa.d.burning_ship ? draw_julia_kernel<ReferenceOrbit<true>> : draw_julia_kernel<ReferenceOrbit<false>>;
        break;
      case 3: kernel = draw_julia_kernel<PowerOrbit<3>>; break;
      case 4: kernel = draw_julia_kernel<PowerOrbit<4>>; break;
      case 5: kernel = draw_julia_kernel<PowerOrbit<5>>; break;
      case 6: kernel = draw_julia_kernel<PowerOrbit<6>>; break;
      case 7: kernel = draw_julia_kernel<PowerOrbit<7>>; break;
      default: kernel = draw_julia_kernel<PowerOrbit<8>>; break;
    }
  }
  hipLaunchKernelGGL(kernel, dim3((pa.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
