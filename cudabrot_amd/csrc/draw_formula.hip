// draw_formula.hip -- the formula render (include/cudabrot_amd.h, "Formula step"): a projected render, a
// Julia render or a palette render of either whose step is another member of the quadratic family -- tricorn, Celtic,
// buffalo, perpendicular, Celtic tricorn -- which differs from the reference's step by a sign or an absolute value in nr
// or ni (device_math.h, formula_step).  Sample stream, iteration, escape index, accept filter, replayed points,
// projection, binning and the palette's weights are those renders', unchanged; like the Multibrot step a formula has no
// cardioid or bulb rejection and no interior map.
//
// Kernels
//   draw_formula_simple_kernel          the definition verbatim, one lane per reference thread in lock-step, no
//                                       early-out; code, Julia-or-not and table-or-not are run-time arguments.
//                                       Validation baseline (cb_debug_last_draw_kernel 17).
//   draw_formula_kernel<F, kJulia, kPalette>  the product kernel (16): the round scheduler of draw_rounds.h with
//                                       PlotMode, JuliaMode or PaletteMode of draw_plot.h over FormulaOrbit<F>, one
//                                       instance per code, per source of c and per sink: 5 x 2 x 2 = 20.  Same
//                                       histogram, generator states and counters (but skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

namespace {

// The kernel's arguments read afresh, as draw_common.h's fresh_args reads a DrawArgs: what an accepted orbit alone needs
// (the table, c's columns of the matrix) is loaded where it is used and holds no scalar register across the loops.
typedef const FormulaArgs __attribute__((address_space(4))) *FormulaKernelArgs;
__device__ __forceinline__ FormulaKernelArgs fresh_formula_args() {
  FormulaKernelArgs p = (FormulaKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_formula_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_formula_simple_kernel(FormulaArgs fa) {
  const PaletteArgs &pl = fa.pl;
  const ProjectArgs &pa = pl.ja.pa;
  const DrawArgs &a = pa.d;
  const int f = fa.formula;
  const bool julia = pl.julia != 0;
  const bool table = fa.palette != 0;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);  // z_0, and c too unless c is fixed
      const double imag = sample_coordinate(rng);
      const double c_re = julia ? pl.ja.c[0] : real;
      const double c_im = julia ? pl.ja.c[1] : imag;
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
      const FormulaKernelArgs now = fresh_formula_args();
      // with a table: min_iter <= k < max_iter == n_entries, and 0 <= k; without one: weight 1 in the one plane there is
      const uint32_t entry = table ? now->pl.lut[k] : 1u;
      const double ku = project_constant(now->pl.ja.pa.p[2], now->pl.ja.pa.p[3], c_re, c_im);
      const double kv = project_constant(now->pl.ja.pa.p[6], now->pl.ja.pa.p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = formula_step(f, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          unsigned long long *plane = a.hist;  // of weight j
          for (int j = 0; j < 3; ++j, plane += pl.plane_pixels) {
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
// draw_formula_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with the modes of draw_plot.h over FormulaOrbit<F>, built as draw_project_kernel,
// draw_julia_kernel and draw_palette_kernel build them: a fixed c makes the plot's constant once, before the first round;
// the palette's mode loads an accepted orbit's entry once and does not replay a zero entry.  The early-out's proof uses
// only that the step is a function of z, which every formula is for a given c.

template <int F, bool kJulia, bool kPalette>
__global__ void __launch_bounds__(256) draw_formula_kernel(FormulaArgs fa) {
  using Step = FormulaOrbit<F>;
  const PaletteArgs &pl = fa.pl;
  const ProjectArgs &pa = pl.ja.pa;
  if constexpr (kPalette && kJulia) {
    const double ku = project_constant(pa.p[2], pa.p[3], pl.ja.c[0], pl.ja.c[1]);
    const double kv = project_constant(pa.p[6], pa.p[7], pl.ja.c[0], pl.ja.c[1]);
    PaletteMode<Step, true> mode{{{pa, make_canvas(pa.d), ku, kv}, pl.ja.c[0], pl.ja.c[1]}, pl.lut, pl.plane_pixels};
    run_rounds(pa.d, mode);
  } else if constexpr (kPalette) {
    PaletteMode<Step, false> mode{{{pa, make_canvas(pa.d)}}, pl.lut, pl.plane_pixels};
    run_rounds(pa.d, mode);
  } else if constexpr (kJulia) {
    JuliaMode<Step> mode{{pa, make_canvas(pa.d)}, pl.ja.c[0], pl.ja.c[1]};
    mode.plot.constant(pl.ja.c[0], pl.ja.c[1]);
    run_rounds(pa.d, mode);
  } else {
    PlotMode<Step> mode{{pa, make_canvas(pa.d)}};
    run_rounds(pa.d, mode);
  }
}

namespace {

template <int F>
void (*formula_kernel(bool julia, bool palette))(FormulaArgs) {
  if (palette) return julia ? draw_formula_kernel<F, true, true> : draw_formula_kernel<F, false, true>;
  return julia ? draw_formula_kernel<F, true, false> : draw_formula_kernel<F, false, false>;
}

}  // namespace

hipError_t launch_draw_formula(const FormulaArgs &a, bool lockstep, hipStream_t stream) {
  const ProjectArgs &pa = a.pl.ja.pa;
  const bool julia = a.pl.julia != 0;
  const bool palette = a.palette != 0;
  if (a.formula < CB_FORMULA_TRICORN || a.formula > CB_FORMULA_MAX) return hipErrorInvalidValue;
  if (pa.degree != 2 || pa.d.burning_ship) return hipErrorInvalidValue;  // a formula is a step of its own
  for (int j = 0; julia && j < 2; ++j) {
    if (!(a.pl.ja.c[j] >= -2.0 && a.pl.ja.c[j] <= 2.0)) return hipErrorInvalidValue;  // a NaN fails both comparisons
  }
  // every accepted k indexes the table: the table covers [0, max_iter)
  if (palette && (a.pl.lut == nullptr || pa.d.max_iter < 1 || pa.d.max_iter > CB_PALETTE_MAX_ENTRIES)) {
    return hipErrorInvalidValue;
  }
  if (pa.d.n_threads == 0 || pa.d.samples_per_thread == 0) return hipSuccess;
  void (*kernel)(FormulaArgs) = nullptr;
  if (lockstep) {
    kernel = draw_formula_simple_kernel;
  } else {
    switch (a.formula) {
      case CB_FORMULA_TRICORN: kernel = formula_kernel<CB_FORMULA_TRICORN>(julia, palette); break;
      case CB_FORMULA_CELTIC: kernel = formula_kernel<CB_FORMULA_CELTIC>(julia, palette); break;
      case CB_FORMULA_BUFFALO: kernel = formula_kernel<CB_FORMULA_BUFFALO>(julia, palette); break;
      case CB_FORMULA_PERPENDICULAR: kernel = formula_kernel<CB_FORMULA_PERPENDICULAR>(julia, palette); break;
      default: kernel = formula_kernel<CB_FORMULA_CELTIC_TRICORN>(julia, palette); break;
    }
  }
  hipLaunchKernelGGL(kernel, dim3((pa.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
