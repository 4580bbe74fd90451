// draw_project.hip -- the projected render (include/cudabrot_amd.h, "Projected render"): every recorded
// orbit point is a point (z_re, z_im, c_re, c_im) of a four-dimensional set, and a 2 x 4 matrix P picks the plane it is
// plotted on:
//   K_u = fma(P[0][2], c_re, P[0][3] * c_im)             (once per sample)
//   u   = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u))
// and v likewise from row 1; (u, v) is binned as the reference bins (re, im).  Samples, cardioid / bulb rejection (not
// for the Burning Ship), IterateMandelbrot, the accept filter min <= k < max and the replayed points z_1 .. z_{k+1} are
// the normal render's.
//
// The Multibrot Buddhabrot (include/cudabrot_amd.h, "Multibrot step") is this render with another step:
// ProjectArgs::degree 2 is the reference's step, 3 <= degree <= 8 is z <- z^degree + c, the power made of degree - 1
// multiplications by z (device_math.h), without cardioid or bulb rejection and without the interior map.
//
// Kernels
//   draw_project_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; the
//                               step is a run-time switch.  Validation baseline (cb_debug_last_draw_kernel 9).
//   draw_project_kernel         the product kernel (8), a template over the step: lanes are refilled from their own
//                               subsequence every kRound steps (draw_rounds.h), a new sample is
//                               looked up in the interior map (Mandelbrot step only) and a marked one retired without
//                               iterating, and an orbit found exactly periodic at a chunk boundary is
//                               retired as never-escaping.  Same histogram, generator states and counters (but
//                               skipped_steps).
//   draw_power_simple_kernel    the lock-step kernel of the Multibrot step (11): the degree is a run-time argument and
//                               the step a run-time loop (power_step).
//   draw_power_kernel<D>        its product kernel (10), one instance per degree, the step the unrolled power_step_n<D>.
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// draw_project_simple_kernel, draw_power_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_project_simple_kernel(ProjectArgs pa) {
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
__global__ void __launch_bounds__(256) draw_power_simple_kernel(ProjectArgs pa) {
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

// ------------------------------------------------------------------------------------------------
// draw_project_kernel, draw_power_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode.  Step says two things: the step, and whether it is the Mandelbrot
// step -- only then does NEXT reject cardioid and bulb and look the sample up in the interior map, a marked one retired
// without iterating; every other step iterates whatever is drawn.  (A short run of tested steps inside NEXT, for the 91 %
// of uniform samples that escape within four, was built and measured: slower)  An escape goes through the
// accept filter to REPLAY of z_1 .. z_n, each point projected and binned (device-scope atomics); an exact cycle never
// escapes and is counted as the reference counts it, the steps not made in skipped_steps.  The early-out's proof uses only
// that the step is a function of z, which z^d + c is too.

template <bool kShip>
__global__ void __launch_bounds__(256) draw_project_kernel(ProjectArgs pa) {
  PlotMode<ReferenceOrbit<kShip>> mode{{pa, make_canvas(pa.d)}};
  run_rounds(pa.d, mode);
}

template <int D>
__global__ void __launch_bounds__(256) draw_power_kernel(ProjectArgs pa) {
  PlotMode<PowerOrbit<D>> mode{{pa, make_canvas(pa.d)}};
  run_rounds(pa.d, mode);
}

hipError_t launch_draw_project(const ProjectArgs &a, bool lockstep, hipStream_t stream) {
  const bool power = a.degree != 2;
  if (power && (a.degree < CB_POWER_MIN || a.degree > CB_POWER_MAX || a.d.burning_ship)) return hipErrorInvalidValue;
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  void (*kernel)(ProjectArgs) = nullptr;
  if (lockstep) {
    kernel = power ? draw_power_simple_kernel : draw_project_simple_kernel;
  } else {
    switch (a.degree) {
      case 2: kernel = a.d.burning_ship ? draw_project_kernel<true> : draw_project_kernel<false>; break;
      case 3: kernel = draw_power_kernel<3>; break;
      case 4: kernel = draw_power_kernel<4>; break;
      case 5: kernel = draw_power_kernel<5>; break;
      case 6: kernel = draw_power_kernel<6>; break;
      case 7: kernel = draw_power_kernel<7>; break;
      default: kernel = draw_power_kernel<8>; break;
    }
  }
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
