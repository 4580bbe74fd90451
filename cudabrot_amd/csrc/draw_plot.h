// draw_plot.h -- what the kernels that plot on a plane of the 4-D set share (draw_plot.hip; include/cudabrot_amd.h,
// "Projected render"): the four fused operations of a plotted point, the plot of a replayed point for the modes of
// draw_rounds.h's scheduler, the steps those modes are instantiated with, the modes themselves -- a sampled c, a fixed
// one, the palette render's mode, which builds on either, and the bounded render's (draw_bounded.hip), which the aimed
// render (draw_aim.hip) wraps as it wraps the first two --, and what the launchers of every family that plots share
// (draw_plot.hip, draw_depth.hip, draw_depth_palette.hip): the list of the steps, a step's index and the checks of one.
#pragma once

#include <type_traits>

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
  const PlotArgs &pa;
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

template <int F>
struct FormulaOrbit {  // include/cudabrot_amd.h, "Formula step": the code wave-uniform and the switch gone
  static constexpr bool kMandelbrot = false;
  static __device__ __forceinline__ double step(double cr, double ci, double &r, double &i) {
    return formula_step<F>(cr, ci, r, i);
  }
};

// ---- the palette's entry (include/cudabrot_amd.h, "Palette render") -----------------------------------------------------

constexpr uint32_t kPaletteWeightBits = 0x00ffffffu;  // bits 24-31 of an entry are not read

// weight_j of an entry: plane 0 = R, 1 = G, 2 = B.
__device__ __forceinline__ unsigned long long palette_weight(uint32_t entry, int plane) {
  return (unsigned long long) ((entry >> (8 * plane)) & 0xffu);
}

// ---- the plot modes of draw_rounds.h's scheduler (draw_plot.hip) ---------------------------------------------------------

namespace {

// One step with c = (c_re, c_im), every choice a run-time argument: a formula code, else a degree other than 2, else the
// reference's step or its Burning Ship variant.
__device__ __forceinline__ double bounded_step(int formula, int degree, bool ship, double c_re, double c_im, double &r,
                                               double &i) {
  if (formula != 0) return formula_step(formula, c_re, c_im, r, i);
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

// The interior map (DrawArgs::interior_map), on undoubled coordinates: column floor((c_re + 2) 2^level), row
// floor(|c_im| 2^level), level = interior_shift + 1.  true: every sample of the cell that holds c provably never escapes.
// kAnySample false: c is a sample of the normal stream, for which c_re + 2 is exact, and the column is made from that sum.
// kAnySample true: c is any double in [-2, 2] -- a sample of a cell list (draw_aim.hip) is corner + offset, ONE rounded
// addition, and for c_re > -1 its ulp is finer than that of c_re + 2, so the sum would round, and could round up onto the
// next cell's edge.  The column is then floor(c_re 2^level) + 2 2^level: the scaling by a power of two and the floor are
// both exact, so the cell looked up is the cell that holds c, and the map's proof covers the sample.  For a sample of
// the normal stream both forms give the same column.
template <bool kAnySample = false>
__device__ __forceinline__ bool interior_marked(const DrawArgs &a, double cr, double ci) {
  const int level = (int) a.interior_shift + 1;
  const double x = kAnySample ? __builtin_floor(__builtin_ldexp(cr, level)) + __builtin_ldexp(2.0, level)
                              : __builtin_ldexp(cr + 2.0, level);
  const double y = __builtin_ldexp(__builtin_fabs(ci), level);
  if (!(x >= 0.0)) return false;
  const uint32_t col = (uint32_t) x;
  const uint32_t row = (uint32_t) y;
  if (col >= a.interior_cols || row >= a.interior_rows) return false;
  const uint32_t index = row * a.interior_cols + col;  // < 2.5 * 1.25 * 4^level
  return ((a.interior_map[index >> 3] >> (index & 7u)) & 1u) != 0u;
}


// The mode of a render that samples c (draw_plot.hip has the commentary): z_0 = c, the plot's constant from the sample.
template <class Step>
struct PlotMode {
  Plot plot;

  __device__ __forceinline__ double step(RoundLane &l) { return Step::step(l.cr, l.ci, l.r, l.i); }

  // What becomes of the sample drawn into (l.cr, l.ci).  kAnySample: it may come from another source than the normal
  // stream (draw_aim.hip draws from a cell list), and the map is looked up with the exact column (interior_marked).
  template <bool kAnySample = false>
  __device__ __forceinline__ int drawn(RoundLane &l) {
    if (!Step::kMandelbrot) return kSampleIterate;
    if (in_main_cardioid(l.cr, l.ci) || in_order2_bulb(l.cr, l.ci)) return kSampleRejected;
    const DrawArgs &a = plot.pa.d;
    if (a.interior_map != nullptr && interior_marked<kAnySample>(a, l.cr, l.ci)) return kSampleInterior;  // not iterated
    return kSampleIterate;
  }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return drawn(l);
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    if (!count_escaped(l, plot.pa.d.min_iter, st)) return false;
    plot.constant(l.cr, l.ci);
    return true;
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool) { return count_never_escapes(l, st); }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    plot.point(l.r, l.i, st);
    return false;
  }
};


// The mode of a Julia render (draw_plot.hip has the commentary): z_0 = the sample, c and the plot's constant fixed.
template <class Step>
struct JuliaMode {
  Plot plot;
  const double c_re, c_im;

  __device__ __forceinline__ double step(RoundLane &l) { return Step::step(c_re, c_im, l.r, l.i); }

  template <bool kAnySample = false>
  __device__ __forceinline__ int drawn(RoundLane &) { return kSampleIterate; }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return drawn(l);
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    return count_escaped(l, plot.pa.d.min_iter, st);
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool) { return count_never_escapes(l, st); }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    plot.point(l.r, l.i, st);
    return false;
  }
};


// The mode of a palette render (draw_plot.hip has the commentary): either mode above with another ESCAPED, which loads
// the orbit's entry once, and another plot, which adds each non-zero weight to the pixel of its plane.
template <class Step, bool kJulia>
struct PaletteMode {
  typename std::conditional<kJulia, JuliaMode<Step>, PlotMode<Step>>::type base;
  const uint32_t *const lut;
  const unsigned long long plane_pixels;
  uint32_t entry = 0u;  // of the orbit in REPLAY

  __device__ __forceinline__ double step(RoundLane &l) { return base.step(l); }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) { return base.next(rng, l); }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    // (for a sampled c, PlotMode also makes an accepted orbit's two projection constants here, before the entry is known:
    // a zero-entry orbit pays for those two operations and never uses them)
    const bool accepted = base.escaped(l, st);
    // k = l.end - 1: min_iter <= k < max_iter == n_entries, and 0 <= k
    entry = accepted ? lut[l.end - 1] & kPaletteWeightBits : 0u;
    // (one add on every path: an add of its own in this branch, beside count_escaped's to too_fast in the other, makes the
    // compiler index the counters through memory)
    st.reserved += accepted && entry == 0u ? (unsigned long long) l.end : 0ull;
    return entry != 0u;
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    return base.never_escapes(l, st, cycle);
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const Plot &plot = base.plot;
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    int row, col;
    if (pixel_of(u, v, plot.cv, row, col)) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned long long weight = palette_weight(entry, j);
        if (weight != 0ull) {
          add_to_pixel(plot.pa.d.hist + (unsigned long long) j * plane_pixels, plot.cv, row, col, weight);
          st.increments += weight;
        }
      }
    }
    return false;
  }
};


// The mode of a bounded render (draw_bounded.hip has the commentary): either source of c, the orbits that do not escape
// replayed cycle-compressed, each point with its exact integer weight.
template <class Step, bool kJulia>
struct BoundedMode {
  Plot plot;
  const double c_re, c_im;  // kJulia: the fixed c
  int cyc = 0;              // REPLAY: s, the first cycle point (> max_iter: no cycle)
  int rem = 0;              // REPLAY: weight q + 1 up to z_{s+rem}, q after it
  unsigned long long q = 0ull;

  __device__ __forceinline__ double step(RoundLane &l) {
    return kJulia ? Step::step(c_re, c_im, l.r, l.i) : Step::step(l.cr, l.ci, l.r, l.i);
  }

  template <bool kAnySample = false>
  __device__ __forceinline__ int drawn(RoundLane &) { return kSampleIterate; }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return drawn(l);
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
      l.end = l.saved - 1 + p;
      q = (unsigned long long) ((l.max_iter - l.saved) / p);
      rem = (l.max_iter - l.saved) % p;
      st.reserved += (unsigned long long) (l.max_iter - l.k) + (unsigned long long) (l.max_iter - l.end);
    } else {
      cyc = l.max_iter + 1;  // no cycle seen: all M points with weight 1
      l.end = l.max_iter;
      q = 0ull;
      rem = 0;
    }
    st.never_escaped++;
    st.recorded++;
    st.iterate_steps += (unsigned long long) l.max_iter;
    st.replay_steps += (unsigned long long) l.max_iter;
    if (!kJulia) plot.constant(l.cr, l.ci);
    return true;
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    int row, col;
    if (pixel_of(u, v, plot.cv, row, col)) {
      const unsigned long long w = l.k < cyc ? 1ull : (l.k - cyc <= rem ? q + 1ull : q);
      add_to_pixel(plot.pa.d.hist, plot.cv, row, col, w);
      st.increments += w;
    }
    return false;
  }
};


// ---- the steps, for the launchers ----------------------------------------------------------------------------------------

// Every step there is, in the order of plot_step_index: the reference's, its Burning Ship variant, degrees CB_POWER_MIN ..
// CB_POWER_MAX, codes CB_FORMULA_TRICORN .. CB_FORMULA_MAX.  A family's table of product kernels is CB_PLOT_STEPS(ROW),
// ROW(Step) the family's kernels of one step.
#define CB_PLOT_STEPS(ROW)                                                                                             \
  ROW(ReferenceOrbit<false>) ROW(ReferenceOrbit<true>)                                                                 \
  ROW(PowerOrbit<3>) ROW(PowerOrbit<4>) ROW(PowerOrbit<5>) ROW(PowerOrbit<6>) ROW(PowerOrbit<7>) ROW(PowerOrbit<8>)    \
  ROW(FormulaOrbit<CB_FORMULA_TRICORN>) ROW(FormulaOrbit<CB_FORMULA_CELTIC>) ROW(FormulaOrbit<CB_FORMULA_BUFFALO>)     \
  ROW(FormulaOrbit<CB_FORMULA_PERPENDICULAR>) ROW(FormulaOrbit<CB_FORMULA_CELTIC_TRICORN>)
constexpr int kFirstPowerStep = 2 - CB_POWER_MIN;
constexpr int kFirstFormulaStep = kFirstPowerStep + CB_POWER_MAX + 1 - CB_FORMULA_TRICORN;
constexpr int kPlotSteps = kFirstFormulaStep + CB_FORMULA_MAX + 1;
inline int plot_step_index(const PlotArgs &a) {
  return a.formula != 0 ? kFirstFormulaStep + a.formula
                        : a.degree != 2 ? kFirstPowerStep + a.degree : (a.d.burning_ship != 0 ? 1 : 0);
}

// What every launcher refuses of a PlotArgs, the tables apart: a step that is none of the list's, a fixed c outside
// [-2, 2]^2.
inline bool plot_launch_ok(const PlotArgs &a) {
  const bool power = a.degree != 2;
  const bool ship = a.d.burning_ship != 0;
  if (power && (a.degree < CB_POWER_MIN || a.degree > CB_POWER_MAX)) return false;
  if (a.formula < 0 || a.formula > CB_FORMULA_MAX) return false;
  if (a.formula != 0 && (power || ship)) return false;  // a formula is a step of its own
  if (power && ship) return false;                      // the Multibrot step has no Burning Ship variant
  for (int j = 0; a.julia != 0 && j < 2; ++j) {
    if (!(a.c[j] >= -2.0 && a.c[j] <= 2.0)) return false;  // a NaN fails both comparisons
  }
  return true;
}

}  // namespace

}  // namespace cb
