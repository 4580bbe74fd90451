// draw_plot.h -- what the kernels that plot on a plane of the 4-D set share (draw_project.hip, draw_julia.hip;
// include/cudabrot_amd.h, "Projected render"): the four fused operations of a plotted point, the plot of a replayed point
// for the modes of draw_rounds.h's scheduler, and the steps those modes are instantiated with.
#pragma once

#include "draw_rounds.h"

namespace cb {

// The part of a plotted coordinate that does not depend on z: the two columns of P that multiply c.
__device__ __forceinline__ double project_constant(double pc_re, double pc_im, double cr, double ci) {
  return __builtin_fma(pc_re, cr, pc_im * ci);
}
// One plotted coordinate of the point (r, i): the two columns of P that multiply z, and the constant.
__device__ __forceinline__ double project_point(double pz_re, double pz_im, double r, double i, double k) {
  return __builtin_fma(pz_re, r, __builtin_fma(pz_im, i, k));
}

// What the product kernels share: the plot of a replayed point.  (ku, kv) is c's part of (u, v).
struct Plot {
  const ProjectArgs &pa;
  const Canvas cv;
  double ku = 0.0, kv = 0.0;

  __device__ __forceinline__ void constant(double cr, double ci) {
    ku = project_constant(pa.p[2], pa.p[3], cr, ci);
    kv = project_constant(pa.p[6], pa.p[7], cr, ci);
  }
  __device__ __forceinline__ void point(double r, double i, LaneStats &st) const {
    const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
    const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
    int row, col;
    if (pixel_of(u, v, cv, row, col)) {
      add_to_pixel(pa.d.hist, cv, row, col, 1ull);
      st.increments++;
    }
  }
};

// The steps a plot mode is a template over.  kMandelbrot: the step whose samples c have a cardioid, a bulb and an
// interior map.
template <bool kShip>
struct ReferenceOrbit {
  static constexpr bool kMandelbrot = !kShip;
  static __device__ __forceinline__ double step(double cr, double ci, double &r, double &i) {
    return orbit_step<kShip>(cr, ci, r, i);
  }
};
template <int D>
struct PowerOrbit {  // the degree wave-uniform and the loop gone
  static constexpr bool kMandelbrot = false;
  static __device__ __forceinline__ double step(double cr, double ci, double &r, double &i) {
    return power_step_n<D>(cr, ci, r, i);
  }
};

}  // namespace cb
