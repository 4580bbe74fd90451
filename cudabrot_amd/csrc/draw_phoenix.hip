// draw_phoenix.hip -- the Phoenix render (include/cudabrot_amd.h, "Phoenix render"): a projected render
// (a sampled c, z_0 = c) or a Julia render (a fixed c, z_0 = the sample) whose step has memory,
//   z_{n+1} = z_n^2 + c + p z_{n-1},
// so that an orbit's state is the pair (z, y), y the point before z and y_0 = 0.  One step is mandel_step's four operations
// followed by four fused ones that add p y to (nr, ni), every one a single rounding.  Nothing is rejected: no cardioid, no
// bulb, no interior map, whatever p is.  Escape index, accept filter min <= k < max, the replayed points z_1 .. z_{k+1} and
// the plot of (z_re, z_im, c_re, c_im) under P[2][4] are the projected render's; y is state and never plotted.
//
// Kernels (the number: cb_debug_last_draw_kernel, capi.hip)
//   draw_phoenix_simple_kernel   the definition verbatim, one lane per reference thread in lock-step, no early-out; the
//                                source of c is a run-time argument.  Validation baseline (25).
//   draw_phoenix_kernel<kJulia>  the product kernel (24): the round scheduler of draw_rounds.h with PhoenixMode, one
//                                instance per source of c.  The mode keeps y and the y saved beside the scheduler's saved z
//                                per lane and gives the scheduler its three state hooks: `start` zeroes y where an orbit
//                                begins, for ITERATE and for REPLAY alike, `save` keeps y where z is saved, and `same` makes
//                                the exact-periodicity test compare the whole state.  (z_k == z_saved with another y proves
//                                nothing: the next point differs.)  With the state compared, the proof of DESIGN.md 4.2
//                                holds as it stands: the step is a function of (z, y) for a given c and p.
// Direct device-scope atomics; no workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by
// exactly its samples.
#include "draw_plot.h"

namespace cb {

namespace {

// One step of the state (r, i, yr, yi) with c = (cr, ci) and p = (pr, pi); returns |z|^2 of the new z as it is tested.
// The product kernel's writing: mandel_step, then p y added to what it made.  (mandel_step's own |z|^2 is not used.)
__device__ __forceinline__ double phoenix_step(double cr, double ci, double pr, double pi, double &r, double &i, double &yr,
                                               double &yi) {
  const double zr = r, zi = i;
  (void) mandel_step(cr, ci, r, i);
  r = __builtin_fma(pr, yr, r);
  r = __builtin_fma(-pi, yi, r);
  i = __builtin_fma(pr, yi, i);
  i = __builtin_fma(pi, yr, i);
  yr = zr;
  yi = zi;
  return __builtin_fma(i, i, r * r);
}

// The same operation sequence written out, for the lock-step kernel (as power_step beside power_step_n: two writings of
// one definition).
__device__ __forceinline__ double phoenix_step_written(double cr, double ci, double pr, double pi, double &r, double &i,
                                                       double &yr, double &yi) {
  const double ii = i * i;
  const double t = __builtin_fma(r, r, -ii);
  double nr = cr + t;
  double ni = __builtin_fma(r + r, i, ci);
  nr = __builtin_fma(pr, yr, nr);
  nr = __builtin_fma(-pi, yi, nr);
  ni = __builtin_fma(pr, yi, ni);
  ni = __builtin_fma(pi, yr, ni);
  yr = r;
  yi = i;
  r = nr;
  i = ni;
  return __builtin_fma(ni, ni, nr * nr);
}

// The mode of a Phoenix render: PlotMode (a sampled c) or JuliaMode (a fixed one) of draw_plot.h without rejection or map,
// with the step above and the rest of the orbit's state.
template <bool kJulia>
struct PhoenixMode {
  Plot plot;
  const double c_re, c_im;  // kJulia: the fixed c
  const double p_re, p_im;
  double yr = 0.0, yi = 0.0;    // y: the point before z
  double syr = 0.0, syi = 0.0;  // ITERATE: the y saved beside the scheduler's z_saved

  __device__ __forceinline__ double step(RoundLane &l) {
    return phoenix_step(kJulia ? c_re : l.cr, kJulia ? c_im : l.ci, p_re, p_im, l.r, l.i, yr, yi);
  }
  __device__ __forceinline__ void start(RoundLane &) { yr = yi = 0.0; }
  __device__ __forceinline__ void save(RoundLane &) {
    syr = yr;
    syi = yi;
  }
  __device__ __forceinline__ bool same(RoundLane &) { return same_bits(yr, yi, syr, syi); }

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return kSampleIterate;
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    if (!count_escaped(l, plot.pa.d.min_iter, st)) return false;
    if (!kJulia) plot.constant(l.cr, l.ci);
    return true;
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool) { return count_never_escapes(l, st); }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    plot.point(l.r, l.i, st);
    return false;
  }
};

}  // namespace

// The lock-step kernel: the definition, verbatim.  The sample is z_0, and c too unless c is fixed.
__global__ void __launch_bounds__(256) draw_phoenix_simple_kernel(PhoenixArgs pa) {
  const PlotArgs &q = pa.plot;
  const DrawArgs &a = q.d;
  const bool julia = q.julia != 0;
  const double p_re = pa.p[0], p_im = pa.p[1];
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);
      const double imag = sample_coordinate(rng);
      const double c_re = julia ? q.c[0] : real;
      const double c_im = julia ? q.c[1] : imag;
      st.samples++;
      int k = a.max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag, yr = 0.0, yi = 0.0;
        for (int it = 0; it < a.max_iter; ++it) {
          if (phoenix_step_written(c_re, c_im, p_re, p_im, r, i, yr, yi) > 4.0) {
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
      const double ku = project_constant(q.p[2], q.p[3], c_re, c_im);
      const double kv = project_constant(q.p[6], q.p[7], c_re, c_im);
      double r = real, i = imag, yr = 0.0, yi = 0.0;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = phoenix_step_written(c_re, c_im, p_re, p_im, r, i, yr, yi);
        st.replay_steps++;
        const double u = project_point(q.p[0], q.p[1], r, i, ku);
        const double v = project_point(q.p[4], q.p[5], r, i, kv);
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

// The product kernel.  The body stands in the kernel, not in a function the kernel calls.
template <bool kJulia>
__global__ void __launch_bounds__(256) draw_phoenix_kernel(PhoenixArgs pa) {
  PhoenixMode<kJulia> mode{{pa.plot, make_canvas(pa.plot.d)}, pa.plot.c[0], pa.plot.c[1], pa.p[0], pa.p[1]};
  if (kJulia) mode.plot.constant(pa.plot.c[0], pa.plot.c[1]);
  run_rounds(pa.plot.d, mode);
}

hipError_t launch_draw_phoenix(const PhoenixArgs &a, bool lockstep, hipStream_t stream) {
  const PlotArgs &q = a.plot;
  if (!plot_launch_ok(q)) return hipErrorInvalidValue;
  if (q.degree != 2 || q.formula != 0 || q.d.burning_ship != 0 || q.palette != 0 || q.lut != nullptr) {
    return hipErrorInvalidValue;
  }
  for (int j = 0; j < 2; ++j) {
    if (!(a.p[j] >= -2.0 && a.p[j] <= 2.0)) return hipErrorInvalidValue;  // a NaN fails both comparisons
  }
  if (q.d.n_threads == 0 || q.d.samples_per_thread == 0) return hipSuccess;
  void (*kernel)(PhoenixArgs) = lockstep       ? draw_phoenix_simple_kernel
                                : q.julia != 0 ? draw_phoenix_kernel<true>
                                               : draw_phoenix_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((q.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
