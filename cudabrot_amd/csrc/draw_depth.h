// draw_depth.h -- what the kernels that bin along a third row share (draw_depth.hip, draw_depth_palette.hip;
// include/cudabrot_amd.h, "Depth render"): the lock-step kernels' step, the arguments read afresh, the slice of a depth, the
// launcher's checks, and DepthMode, the mode of draw_rounds.h's scheduler that both product kernels run.
#pragma once

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
// iterate loop.  (A DepthPaletteArgs begins with its DepthArgs: the same pointer serves its kernels.)
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

// What both launchers refuse of a DepthArgs, the table apart: whatever launch_draw_plot refuses of p (draw_plot.h,
// plot_launch_ok), slices out of range, a delta that is not positive, a plane_pixels that is not w * h.
inline bool depth_launch_ok(const DepthArgs &da) {
  const PlotArgs &a = da.p;
  // every slice the kernel can compute is a plane of the histogram: 1 <= N, and the window and its step are what
  // slice_of divides by
  return plot_launch_ok(a) && da.slices >= 1 && da.slices <= CB_DEPTH_MAX_SLICES && da.delta > 0.0 && a.d.w > 0 &&
         a.d.h > 0 && da.plane_pixels == (unsigned long long) a.d.w * (unsigned long long) a.d.h;
}

// The round scheduler of draw_rounds.h with DepthMode: PlotMode (a sampled c) or JuliaMode (a fixed one) of draw_plot.h
// with another ESCAPED and another plot.  The lane keeps K_d beside the base's K_u and K_v through the replay: two more
// vector registers.  The depth row's columns of c are read from the argument segment in ESCAPED, where they are used; the
// two columns of z, the window and the slice count are wave-uniform operands of the replayed point, as the matrix and
// the canvas are.  The plane of the add is one 64-bit multiply-add on the address: the atomic itself is the projected
// render's, one device-scope add per point, into N times the address range.
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

}  // namespace cb
