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
#include "draw_plot.h"

namespace cb {

namespace {

// One step with c = (c_re, c_im): a formula's, else degree 2 is the reference's step or its Burning Ship variant, else
// the Multibrot step.
__device__ __forceinline__ double depth_step(int formula, int degree, bool ship, double c_re, double c_im, double &r,
                                             double &i) {
  if (formula != 0) return formula_step(formula, c_re, c_im, r, i);
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

// The kernel's arguments read afresh, as draw_plot.hip's fresh_plot_args reads a PlotArgs: what an accepted orbit alone
// needs (c's columns of the matrix and of the depth row; in the lock-step kernel the rest of the depth's parameters too,
// whose scalar registers would otherwise spill) is loaded where it is used and holds no scalar register across the
// iterate loop.
typedef const DepthArgs __attribute__((address_space(4))) *DepthKernelArgs;
__device__ __forceinline__ DepthKernelArgs fresh_depth_args() {
  DepthKernelArgs p = (DepthKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// The slice a depth falls in: the reference's binning of `im` (pixel_of's row arithmetic) with the window [min, min + N
// delta) in the place of the canvas's rows.  true and s if the point is in depth.
__device__ __forceinline__ bool slice_of(double d, double min, double delta, double inv_delta, int pow2, int slices,
                                         int &s) {
  if (d < min) return false;
  const double fd = d - min;
  // (int) of a double: v_cvt_i32_f64 saturates where x86 yields INT_MIN; both fail the bounds test.
  s = pow2 ? (int) (fd * inv_delta) : (int) (fd / delta);
  return (s >= 0) && (s < slices);
}

}  // namespace

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
// The round scheduler of draw_rounds.h with DepthMode: PlotMode (a sampled c) or JuliaMode (a fixed one) of draw_plot.h
// with another ESCAPED and another plot.  The lane keeps K_d beside the base's K_u and K_v through the replay: two more
// vector registers.  The depth row's columns of c are read from the argument segment in ESCAPED, where they are used; the
// two columns of z, the window and the slice count are wave-uniform operands of the replayed point, as the matrix and
// the canvas are.  The plane of the add is one 64-bit multiply-add on the address: the atomic itself is the projected
// render's, one device-scope add per point, into N times the address range.
//
// The body stands in the kernel, not in a function the kernel calls.

namespace {

template <class Step, bool kJulia>
struct DepthMode {
  typename std::conditional<kJulia, JuliaMode<Step>, PlotMode<Step>>::type base;
  const DepthArgs &da;
  double kd = 0.0;  // c's part of d: of the orbit in REPLAY, or of the fixed c

  __device__ __forceinline__ double step(RoundLane &l) { return base.step(l); }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) { return base.next(rng, l); }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    const bool accepted = base.escaped(l, st);
    if constexpr (!kJulia) {
      if (accepted) {
        const DepthKernelArgs now = fresh_depth_args();
        kd = project_constant(now->row[2], now->row[3], l.cr, l.ci);
      }
    }
    return accepted;
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    return base.never_escapes(l, st, cycle);
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const Plot &plot = base.plot;
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    const double d = project_point(da.row[0], da.row[1], l.r, l.i, kd);
    int row, col, s;
    if (pixel_of(u, v, plot.cv, row, col) && slice_of(d, da.min, da.delta, da.inv_delta, da.pow2, da.slices, s)) {
      add_to_pixel(plot.pa.d.hist + (unsigned long long) s * da.plane_pixels, plot.cv, row, col, 1ull);
      st.increments++;
    }
    return false;
  }
};

}  // namespace

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

// The product kernels of one step: [fixed c].
struct StepKernels {
  DepthKernel by[2];
};
template <class Step>
constexpr StepKernels step_kernels() {
  return {{draw_depth_kernel<Step, false>, draw_depth_kernel<Step, true>}};
}

// Every product kernel there is, by step, in draw_plot.hip's order: the reference's, its Burning Ship variant, degrees
// CB_POWER_MIN .. CB_POWER_MAX, codes CB_FORMULA_TRICORN .. CB_FORMULA_MAX.
constexpr int kFirstPowerStep = 2 - CB_POWER_MIN;
constexpr int kFirstFormulaStep = kFirstPowerStep + CB_POWER_MAX + 1 - CB_FORMULA_TRICORN;
constexpr StepKernels kDepthKernels[] = {
    step_kernels<ReferenceOrbit<false>>(), step_kernels<ReferenceOrbit<true>>(),
    step_kernels<PowerOrbit<3>>(), step_kernels<PowerOrbit<4>>(), step_kernels<PowerOrbit<5>>(),
    step_kernels<PowerOrbit<6>>(), step_kernels<PowerOrbit<7>>(), step_kernels<PowerOrbit<8>>(),
    step_kernels<FormulaOrbit<CB_FORMULA_TRICORN>>(), step_kernels<FormulaOrbit<CB_FORMULA_CELTIC>>(),
    step_kernels<FormulaOrbit<CB_FORMULA_BUFFALO>>(), step_kernels<FormulaOrbit<CB_FORMULA_PERPENDICULAR>>(),
    step_kernels<FormulaOrbit<CB_FORMULA_CELTIC_TRICORN>>(),
};
static_assert(sizeof(kDepthKernels) / sizeof(kDepthKernels[0]) == kFirstFormulaStep + CB_FORMULA_MAX + 1, "one row per step");

}  // namespace

hipError_t launch_draw_depth(const DepthArgs &da, bool lockstep, hipStream_t stream) {
  const PlotArgs &a = da.p;
  const bool power = a.degree != 2;
  const bool ship = a.d.burning_ship != 0;
  const bool julia = a.julia != 0;
  if (power && (a.degree < CB_POWER_MIN || a.degree > CB_POWER_MAX)) return hipErrorInvalidValue;
  if (a.formula < 0 || a.formula > CB_FORMULA_MAX) return hipErrorInvalidValue;
  if (a.formula != 0 && (power || ship)) return hipErrorInvalidValue;  // a formula is a step of its own
  if (power && ship) return hipErrorInvalidValue;                      // the Multibrot step has no Burning Ship variant
  for (int j = 0; julia && j < 2; ++j) {
    if (!(a.c[j] >= -2.0 && a.c[j] <= 2.0)) return hipErrorInvalidValue;  // a NaN fails both comparisons
  }
  if (a.palette != 0 || a.lut != nullptr) return hipErrorInvalidValue;  // no table: 3 N planes are out of scope
  // every slice the kernel can compute is a plane of the histogram: 1 <= N, and the window and its step are what
  // slice_of divides by
  if (da.slices < 1 || da.slices > CB_DEPTH_MAX_SLICES || !(da.delta > 0.0) || a.d.w <= 0 || a.d.h <= 0 ||
      da.plane_pixels != (unsigned long long) a.d.w * (unsigned long long) a.d.h) {
    return hipErrorInvalidValue;
  }
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  DepthKernel kernel = nullptr;
  if (lockstep) {
    kernel = draw_depth_simple_kernel;
  } else {
    const int step = a.formula != 0 ? kFirstFormulaStep + a.formula : power ? kFirstPowerStep + a.degree : (ship ? 1 : 0);
    kernel = kDepthKernels[step].by[julia];
  }
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, da);
  return hipGetLastError();
}

}  // namespace cb
