// draw_power.hip -- the Multibrot Buddhabrot (include/cudabrot_amd.h, "Multibrot step"): the projected
// render of draw_project.hip with the step z <- z^d + c, 3 <= d <= 8, the power made of d - 1 multiplications by z
// (device_math.h).  Samples, IterateMandelbrot, the accept filter min <= k < max, the replayed points z_1 .. z_{k+1}, the
// projection P and pixel_of are the projected render's; there is no cardioid or bulb rejection and no interior map.
//
// Kernels
//   draw_power_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; the
//                             degree is a run-time argument and the step a run-time loop (power_step).  Validation
//                             baseline (cb_debug_last_draw_kernel 11).
//   draw_power_kernel<D>      the product kernel (10), one instance per degree: a mode of the round scheduler
//                             (draw_rounds.h) whose step is the unrolled power_step_n<D>; an orbit found exactly
//                             periodic at a chunk boundary is retired as never-escaping.  Same histogram,
//                             generator states and counters (but skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_rounds.h"

namespace cb {

namespace {

// The plot of draw_project.hip: the sample's part of a coordinate, and the coordinate of the point (r, i).
__device__ __forceinline__ double plot_constant(double pc_re, double pc_im, double cr, double ci) {
  return __builtin_fma(pc_re, cr, pc_im * ci);
}
__device__ __forceinline__ double plot_point(double pz_re, double pz_im, double r, double i, double k) {
  return __builtin_fma(pz_re, r, __builtin_fma(pz_im, i, k));
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_power_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_power_simple_kernel(PowerArgs pa) {
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
      const double ku = plot_constant(pa.p[2], pa.p[3], real, imag);
      const double kv = plot_constant(pa.p[6], pa.p[7], real, imag);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = power_step(d, real, imag, r, i);
        st.replay_steps++;
        const double u = plot_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = plot_point(pa.p[4], pa.p[5], r, i, kv);
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
// draw_power_kernel<D>: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode: NEXT draws a uniform sample and iterates it, whatever it is; the
// step is the mode's own (power_step_n<D>, the degree wave-uniform and the loop gone); an escape goes through the accept
// filter to REPLAY of z_1 .. z_n, each point projected and binned (device-scope atomics); an exact cycle never escapes
// and is counted as the definition counts it, the steps not made in skipped_steps.  The early-out's proof uses only that
// the step is a function of z, which z^d + c is.

namespace {

template <int D>
struct PowerMode {
  const PowerArgs &pa;
  const Canvas cv;
  double ku = 0.0, kv = 0.0;  // REPLAY: the sample's part of (u, v)

  __device__ __forceinline__ double step(RoundLane &l) { return power_step_n<D>(l.cr, l.ci, l.r, l.i); }

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    l.cr = sample_coordinate(rng);
    l.ci = sample_coordinate(rng);
    return kSampleIterate;
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    st.iterate_steps += (unsigned long long) l.end;
    if (l.end - 1 < pa.d.min_iter) {
      st.too_fast++;
      return false;
    }
    st.recorded++;
    st.replay_steps += (unsigned long long) l.end;
    ku = plot_constant(pa.p[2], pa.p[3], l.cr, l.ci);
    kv = plot_constant(pa.p[6], pa.p[7], l.cr, l.ci);
    return true;
  }

  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool) {
    st.never_escaped++;
    st.iterate_steps += (unsigned long long) l.max_iter;
    st.reserved += (unsigned long long) (l.max_iter - l.k);  // 0 at k == max_iter
    return false;
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const double u = plot_point(pa.p[0], pa.p[1], l.r, l.i, ku);
    const double v = plot_point(pa.p[4], pa.p[5], l.r, l.i, kv);
    int row, col;
    if (pixel_of(u, v, cv, row, col)) {
      add_to_pixel(pa.d.hist, cv, row, col, 1ull);
      st.increments++;
    }
    return false;
  }
};

}  // namespace

template <int D>
__global__ void __launch_bounds__(256) draw_power_kernel(PowerArgs pa) {
  PowerMode<D> mode{pa, make_canvas(pa.d)};
  run_rounds(pa.d, mode);
}

hipError_t launch_draw_power(const PowerArgs &a, bool lockstep, hipStream_t stream) {
  if (a.degree < CB_POWER_MIN || a.degree > CB_POWER_MAX) return hipErrorInvalidValue;
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const uint32_t blocks = (a.d.n_threads + 255u) / 256u;
  if (lockstep) {
    hipLaunchKernelGGL(draw_power_simple_kernel, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  switch (a.degree) {
    case 3: hipLaunchKernelGGL(draw_power_kernel<3>, dim3(blocks), dim3(256), 0, stream, a); break;
    case 4: hipLaunchKernelGGL(draw_power_kernel<4>, dim3(blocks), dim3(256), 0, stream, a); break;
    case 5: hipLaunchKernelGGL(draw_power_kernel<5>, dim3(blocks), dim3(256), 0, stream, a); break;
    case 6: hipLaunchKernelGGL(draw_power_kernel<6>, dim3(blocks), dim3(256), 0, stream, a); break;
    case 7: hipLaunchKernelGGL(draw_power_kernel<7>, dim3(blocks), dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL(draw_power_kernel<8>, dim3(blocks), dim3(256), 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace cb
