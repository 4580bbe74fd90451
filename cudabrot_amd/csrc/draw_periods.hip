// draw_periods.hip -- the period-palette render (include/cudabrot_amd.h, "Period-palette render"): the
// bounded render (draw_bounded.hip) with a table keyed by the PERIOD of the cycle a bounded orbit falls onto.  Which samples
// are bounded, their M points, the step, the source of c, the projection and the binning are the bounded render's.  The
// period of a bounded sample is a tolerant return time from z_M: the orbit is continued past z_M, without an escape test,
// and the period is the least j in 1 .. J = n_entries - 1 with
//   dr = re(z_{M+j}) - re(z_M), di = im(z_{M+j}) - im(z_M), fma(dr, dr, di * di) <= eps
// or 0 if there is none.  Each of the M points then adds the three weights of lut[period] to its pixel of three planes.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_periods_simple_kernel     the definition verbatim, one lane per reference thread in lock-step: iterate to M,
//                                  continue up to J steps for the period, load the entry, replay all M points.  Step,
//                                  degree / formula and the source of c are run-time arguments.  Validation baseline (29).
//   draw_periods_kernel<Step, kJulia>
//                                  the product kernel (28): the round scheduler of draw_rounds.h with PeriodMode, which is
//                                  BoundedMode's cycle compression with a SEARCH pass chained in front of its REPLAY
//                                  (draw_rounds.h, round_again).  One instance per step and per source of c: 13 x 2 = 26.
// The table is read once per bounded orbit, from global memory.  No workspace, no carry, no LDS.
#include "draw_plot.h"

namespace cb {

namespace {

__device__ __forceinline__ double periods_step(int formula, int degree, bool ship, double c_re, double c_im, double &r,
                                               double &i) {
  if (formula != 0) return formula_step(formula, c_re, c_im, r, i);
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

// The return test of the definition, in its operation order.  A NaN compares false.
__device__ __forceinline__ bool period_returned(double r, double i, double pr, double pi, double eps) {
  const double dr = r - pr;
  const double di = i - pi;
  return __builtin_fma(dr, dr, di * di) <= eps;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_periods_simple_kernel: the definition, verbatim, written out
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_periods_simple_kernel(PeriodArgs qa) {
  const PlotArgs &pa = qa.p;
  const DrawArgs &a = pa.d;
  const int f = pa.formula;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pa.julia != 0;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter > 0 ? a.max_iter : 0;
  const int max_period = qa.n_entries - 1;  // J
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
      double r = real, i = imag;
      for (int it = 0; it < max_iter; ++it) {
        if (periods_step(f, d, ship, c_re, c_im, r, i) > 4.0) {
          k = it;
          break;
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
      // the period: the least j with z_{M+j} within eps of z_M, no escape test, counted nowhere
      int period = 0;
      {
        const double probe_r = r, probe_i = i;
        for (int j = 1; j <= max_period; ++j) {
          (void) periods_step(f, d, ship, c_re, c_im, r, i);
          if (period_returned(r, i, probe_r, probe_i, qa.eps)) {
            period = j;
            break;
          }
        }
      }
      const uint32_t entry = qa.lut[period];
      const double ku = project_constant(pa.p[2], pa.p[3], c_re, c_im);
      const double kv = project_constant(pa.p[6], pa.p[7], c_re, c_im);
      r = real;
      i = imag;
      for (int it = 0; it < max_iter; ++it) {
        (void) periods_step(f, d, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const unsigned long long weight = palette_weight(entry, j);
            if (weight != 0ull) {
              add_to_pixel(a.hist + (unsigned long long) j * qa.plane_pixels, cv, row, col, weight);
              st.increments += weight;
            }
          }
        }
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_periods_kernel: cycle-compressed, the search a scheduled pass in front of the replay
// ------------------------------------------------------------------------------------------------
//
// BoundedMode (draw_bounded.hip) with two passes after never_escapes instead of one:
//   SEARCH   a REPLAY-like pass that `start` places at the point the lane holds instead of z_0: z_s (= the saved point, bit
//            for bit z_k) if an exact cycle was found, else z_M.  It walks rem = (M - s) mod p steps to the PROBE -- 0 steps
//            without a cycle, or with rem == 0, where the origin is the probe -- and then up to J steps, and `point`
//            compares each with the probe as the definition does; the first return ends the pass.  If z_k == z_s bit for
//            bit, z_M is the cycle point z_{s+rem} bit for bit, and z_{M+j} what the step makes of it: the walk from z_s
//            meets the probe after rem steps and every z_{M+j} after that.  Origin and probe live in the lane's (sr, si),
//            which ITERATE no longer needs.
//   REPLAY   `again` loads lut[period] once when SEARCH ends.  A zero entry: the replay is booked into skipped_steps and
//            the lane takes its next sample.  Else BoundedMode's replay, each weight multiplied by the entry's three.
// The search's steps are made in rounds like every other phase's, while the other lanes go on with theirs; they are
// counted nowhere.

namespace {

template <class Step, bool kJulia>
struct PeriodMode {
  Plot plot;
  const PeriodArgs &qa;
  const double c_re, c_im;  // kJulia: the fixed c
  int cyc = 0;              // REPLAY: s, the first cycle point (> max_iter: no cycle)
  int rem = 0;              // SEARCH: steps to the probe; REPLAY: weight q + 1 up to z_{s+rem}, q after it
  unsigned long long q = 0ull;
  int replay_end = 0;     // the `end` of the REPLAY that follows SEARCH
  bool search = false;    // the pass in progress is SEARCH
  uint32_t entry = 0u;    // SEARCH: the period found so far (0: none); REPLAY: lut[period]

  __device__ __forceinline__ double step(RoundLane &l) {
    return kJulia ? Step::step(c_re, c_im, l.r, l.i) : Step::step(l.cr, l.ci, l.r, l.i);
  }

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return kSampleIterate;
  }

  // run_rounds has set z = z_0: SEARCH starts from its origin instead
  __device__ __forceinline__ void start(RoundLane &l) {
    if (search) {
      l.r = l.sr;
      l.i = l.si;
    }
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {  // nothing recorded
    st.too_fast++;
    st.iterate_steps += (unsigned long long) l.end;
    return false;
  }

  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    if (cycle) {  // z_k == z_saved: p = k - saved (a multiple of the least period)
      const int p = l.k - l.saved;
      cyc = l.saved;
      replay_end = l.saved - 1 + p;
      q = (unsigned long long) ((l.max_iter - l.saved) / p);
      rem = (l.max_iter - l.saved) % p;
      st.reserved += (unsigned long long) (l.max_iter - l.k) + (unsigned long long) (l.max_iter - replay_end);
    } else {
      cyc = l.max_iter + 1;  // no cycle seen: all M points with weight 1
      replay_end = l.max_iter;
      q = 0ull;
      rem = 0;
      l.sr = l.r;  // the origin of SEARCH: z_M
      l.si = l.i;
    }
    st.never_escaped++;
    st.recorded++;
    st.iterate_steps += (unsigned long long) l.max_iter;
    st.replay_steps += (unsigned long long) l.max_iter;
    if (!kJulia) plot.constant(l.cr, l.ci);
    search = true;
    entry = 0u;
    l.end = rem + (qa.n_entries - 1);
    return true;
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    if (search) {
      if (l.k > rem) {
        if (period_returned(l.r, l.i, l.sr, l.si, qa.eps)) {
          entry = (uint32_t) (l.k - rem);
          return true;
        }
      } else if (l.k == rem) {  // the probe z_M (rem == 0: the origin is the probe, and k >= 1 never comes here)
        l.sr = l.r;
        l.si = l.i;
      }
      return false;
    }
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    int row, col;
    if (pixel_of(u, v, plot.cv, row, col)) {
      const unsigned long long w = l.k < cyc ? 1ull : (l.k - cyc <= rem ? q + 1ull : q);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned long long weight = palette_weight(entry, j) * w;
        if (weight != 0ull) {
          add_to_pixel(plot.pa.d.hist + (unsigned long long) j * qa.plane_pixels, plot.cv, row, col, weight);
          st.increments += weight;
        }
      }
    }
    return false;
  }

  // A pass has ended.  SEARCH: the entry of the period found, and the REPLAY unless it is zero.  REPLAY: the sample is done.
  __device__ __forceinline__ bool again(RoundLane &l, LaneStats &st) {
    if (!search) return false;
    search = false;
    entry = qa.lut[entry] & kPaletteWeightBits;
    st.reserved += entry == 0u ? (unsigned long long) replay_end : 0ull;
    l.end = replay_end;
    return entry != 0u;
  }
};

}  // namespace

// The body stands in the kernel, not in a function the kernel calls.
template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_periods_kernel(PeriodArgs qa) {
  PeriodMode<Step, kJulia> mode{{qa.p, make_canvas(qa.p.d)}, qa, qa.p.c[0], qa.p.c[1]};
  if constexpr (kJulia) mode.plot.constant(qa.p.c[0], qa.p.c[1]);
  run_rounds(qa.p.d, mode);
}

namespace {

typedef void (*PeriodKernel)(PeriodArgs);

// The product kernels of one step, [fixed c], and every one there is, by step (draw_plot.h, plot_step_index).
struct PeriodStepKernels {
  PeriodKernel by[2];
};
#define CB_ROW(Step) {{draw_periods_kernel<Step, false>, draw_periods_kernel<Step, true>}},
constexpr PeriodStepKernels kPeriodKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kPeriodKernels) / sizeof(kPeriodKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_periods(const PeriodArgs &a, bool lockstep, hipStream_t stream) {
  if (!plot_launch_ok(a.p) || a.p.palette != 0 || a.p.lut != nullptr) return hipErrorInvalidValue;
  if (a.lut == nullptr || a.n_entries < 2 || a.n_entries > CB_PERIOD_MAX_ENTRIES) return hipErrorInvalidValue;
  if (!(a.eps >= 0.0) || !(a.eps <= 0x1.fffffffffffffp+1023)) return hipErrorInvalidValue;  // negative, infinite, a NaN
  if (a.plane_pixels != (unsigned long long) a.p.d.w * (unsigned long long) a.p.d.h) return hipErrorInvalidValue;
  if (a.p.d.n_threads == 0 || a.p.d.samples_per_thread == 0) return hipSuccess;
  const PeriodKernel kernel =
      lockstep ? draw_periods_simple_kernel : kPeriodKernels[plot_step_index(a.p)].by[a.p.julia != 0];
  hipLaunchKernelGGL(kernel, dim3((a.p.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
