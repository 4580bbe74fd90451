// draw_aim.hip -- the aimed render (include/cudabrot_amd.h, "Aimed render"): a cropped plotted render
// sampled only from the cells of its sample plane whose samples reach the canvas.  It is an UN-AIMED render -- a projected
// render (draw_plot.hip: matrix P, a step of CB_PLOT_STEPS, c sampled or fixed) or a bounded one (draw_bounded.hip), one
// plane, no table -- with the focused render's (draw_focus.hip) source and sink in front of and behind it:
//   source  uniform   the normal stream: 4 XORWOW draws per sample over [-2, 2)^2
//           cells     6 draws per sample: a cell of the list (two draws), a point of that cell (four)
//   sink    histogram what the un-aimed render adds, with its weights
//           mask      the probe: the replay stops at the first plotted point pixel_of bins and sets the bit of the cell that
//                     holds the SAMPLE -- c when c is sampled, z_0 when c is fixed
// From the sample on everything is the un-aimed render's: cardioid / bulb rejection and the interior map for the Mandelbrot
// step on a sampled c of the escaping kind only, the accept filter, the cycle-compressed weights of a bounded orbit.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_aim_simple_kernel            the definition verbatim, one lane per reference thread in lock-step: source, sink,
//                                     step, source of c and kind are run-time arguments; no early-out, no map, weight 1
//                                     everywhere.  Validation baseline (31).
//   draw_aim_kernel<Step, kJulia, kBounded>
//                                     the aimed draw (30): the round scheduler of draw_rounds.h with the un-aimed render's
//                                     mode (PlotMode, JuliaMode, BoundedMode of draw_plot.h) wrapped in AimMode, which
//                                     replaces the draw of NEXT and nothing else.  cells == null: the uniform source, a
//                                     wave-uniform branch in NEXT only -- the un-aimed render bit for bit.  13 x 2 x 2 = 52.
//   draw_aim_probe_kernel<kJulia, kBounded>
//                                     the probe (30 too): uniform source, mask sink, the step a run-time argument
//                                     (bounded_step) -- it runs for tens of passes once per render.  4 instances.
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_cells.h"
#include "draw_plot.h"

namespace cb {

namespace {

// The kernel's arguments read afresh, as draw_plot.hip's fresh_plot_args reads a PlotArgs: what one sample's draw or one
// accepted orbit alone needs (the grid, c's columns of the matrix) is loaded where it is used and holds no scalar register
// across the loops.
typedef const AimArgs __attribute__((address_space(4))) *AimKernelArgs;
__device__ __forceinline__ AimKernelArgs fresh_aim_args() {
  AimKernelArgs p = (AimKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_aim_simple_kernel: the definition, verbatim, written out
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_aim_simple_kernel(AimArgs aa) {
  const PlotArgs &pa = aa.p;
  const DrawArgs &a = pa.d;
  const int f = pa.formula;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pa.julia != 0;
  const bool bounded = aa.bounded != 0;
  const bool from_cells = aa.cells != nullptr;
  const bool to_mask = aa.mask != nullptr;
  // the Mandelbrot step on a sampled c, escaping orbits: cardioid and bulb
  const bool rejects = !bounded && !julia && f == 0 && d == 2 && !ship;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter > 0 ? a.max_iter : 0;
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      double real, imag;  // the sample: z_0, and c too unless c is fixed
      if (from_cells) {
        next_sample<true>(*fresh_aim_args(), rng, real, imag);
      } else {
        next_sample<false>(aa, rng, real, imag);
      }
      const double c_re = julia ? pa.c[0] : real;
      const double c_im = julia ? pa.c[1] : imag;
      st.samples++;
      if (rejects && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      int k = max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < max_iter; ++it) {
          if (bounded_step(f, d, ship, c_re, c_im, r, i) > 4.0) {
            k = it;
            break;
          }
        }
      }
      int n;  // the plotted orbit: z_1 .. z_n
      if (bounded) {
        if (k < max_iter) {  // escaped at z_{k+1}: nothing plotted
          st.too_fast++;
          st.iterate_steps += (unsigned long long) k + 1ull;
          continue;
        }
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) max_iter;
        n = max_iter;
      } else {
        if (k >= max_iter) {
          st.never_escaped++;
          st.iterate_steps += (unsigned long long) max_iter;
          continue;
        }
        st.iterate_steps += (unsigned long long) k + 1ull;
        if (k < a.min_iter) {
          st.too_fast++;
          continue;
        }
        n = k + 1;
      }
      if (!to_mask) st.recorded++;
      const AimKernelArgs now = fresh_aim_args();
      const double ku = project_constant(now->p.p[2], now->p.p[3], c_re, c_im);
      const double kv = project_constant(now->p.p[6], now->p.p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it < n; ++it) {
        (void) bounded_step(f, d, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
          if (to_mask) {  // the first in-canvas point: the sample's cell reaches the canvas
            mark_cell(*fresh_aim_args(), real, imag);
            st.recorded++;
            break;
          }
          add_to_pixel(a.hist, cv, row, col, 1ull);
          st.increments++;
        }
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_aim_kernel: the un-aimed render's mode behind another source
// ------------------------------------------------------------------------------------------------
//
// AimMode wraps the un-aimed render's mode the way PaletteMode wraps its base: step, ESCAPED, the never-escaping case and
// the plot are the base's, unchanged.  NEXT draws from the cell list -- or, with no list, from the normal stream: the branch
// is on a kernel argument, wave-uniform -- and then asks the base what becomes of the sample (`drawn`: cardioid, bulb and the
// interior map for PlotMode with the Mandelbrot step, nothing for the others).

namespace {

template <class Base>
struct AimMode {
  Base base;
  const AimArgs &aa;

  __device__ __forceinline__ double step(RoundLane &l) { return base.step(l); }

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    if (aa.cells != nullptr) {
      next_sample<true>(aa, rng, l.cr, l.ci);
    } else {
      next_sample<false>(aa, rng, l.cr, l.ci);
    }
    return base.template drawn<true>(l);  // a sample of a cell may lie where c_re + 2 rounds: the exact map column
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) { return base.escaped(l, st); }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    return base.never_escapes(l, st, cycle);
  }
  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) { return base.point(l, st); }
};

// The probe's mode: the un-aimed render up to the replay, counted as that render counts it, with the step at run time.
//   escaping kind   an accepted orbit replays z_1 .. z_{k+1};
//   bounded kind    a sample that does not escape replays z_1 .. z_M, cycle-compressed as BoundedMode replays it: z_1 ..
//                   z_{s-1+p} in the naive order, and any later point is bit for bit one of those, so the first in-canvas
//                   point has the naive replay's index.
// The first plotted point that pixel_of bins marks the cell of the sample (l.cr, l.ci), counts the sample in `recorded`,
// gives back the replay steps not made and ends the replay.
template <bool kJulia, bool kBounded>
struct AimProbeMode {
  Plot plot;
  const AimArgs &aa;
  const double c_re, c_im;  // kJulia: the fixed c
  const int formula, degree;
  const bool ship;
  const bool rejects;  // the Mandelbrot step on a sampled c, escaping orbits

  __device__ __forceinline__ double step(RoundLane &l) {
    return bounded_step(formula, degree, ship, kJulia ? c_re : l.cr, kJulia ? c_im : l.ci, l.r, l.i);
  }

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    if (kJulia || kBounded || !rejects) return kSampleIterate;
    if (in_main_cardioid(l.cr, l.ci) || in_order2_bulb(l.cr, l.ci)) return kSampleRejected;
    const DrawArgs &a = plot.pa.d;
    if (a.interior_map != nullptr && interior_marked(a, l.cr, l.ci)) return kSampleInterior;  // not iterated
    return kSampleIterate;
  }

  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    if (kBounded) {  // nothing plotted
      st.too_fast++;
      st.iterate_steps += (unsigned long long) l.end;
      return false;
    }
    if (!count_escaped(l, plot.pa.d.min_iter, st, false)) return false;
    total = l.end;
    if (!kJulia) plot.constant(l.cr, l.ci);
    return true;
  }

  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    if (!kBounded) return count_never_escapes(l, st);
    if (cycle) {  // z_k == z_saved: the transient and ONE period visit every point the orbit has
      st.reserved += (unsigned long long) (l.max_iter - l.k);
      l.end = l.k - 1;
    } else {
      l.end = l.max_iter;
    }
    total = l.max_iter;
    st.never_escaped++;
    st.iterate_steps += (unsigned long long) l.max_iter;
    st.replay_steps += (unsigned long long) l.max_iter;
    if (!kJulia) plot.constant(l.cr, l.ci);
    return true;
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    int row, col;
    if (!pixel_of(u, v, plot.cv, row, col)) return false;
    mark_cell(aa, l.cr, l.ci);
    st.recorded++;
    st.replay_steps -= (unsigned long long) (total - l.k);
    return true;
  }

  int total = 0;  // REPLAY: the steps the naive replay makes when no point is on the canvas
};

}  // namespace

// The bodies stand in the kernels, not in a function the kernels call.
template <class Step, bool kJulia, bool kBounded>
__global__ void __launch_bounds__(256) draw_aim_kernel(AimArgs aa) {
  const PlotArgs &pa = aa.p;
  if constexpr (kBounded) {
    AimMode<BoundedMode<Step, kJulia>> mode{{{pa, make_canvas(pa.d)}, pa.c[0], pa.c[1]}, aa};
    if constexpr (kJulia) mode.base.plot.constant(pa.c[0], pa.c[1]);
    run_rounds(pa.d, mode);
  } else if constexpr (kJulia) {
    AimMode<JuliaMode<Step>> mode{{{pa, make_canvas(pa.d)}, pa.c[0], pa.c[1]}, aa};
    mode.base.plot.constant(pa.c[0], pa.c[1]);
    run_rounds(pa.d, mode);
  } else {
    AimMode<PlotMode<Step>> mode{{{pa, make_canvas(pa.d)}}, aa};
    run_rounds(pa.d, mode);
  }
}

template <bool kJulia, bool kBounded>
__global__ void __launch_bounds__(256) draw_aim_probe_kernel(AimArgs aa) {
  const PlotArgs &pa = aa.p;
  const bool ship = pa.d.burning_ship != 0;
  AimProbeMode<kJulia, kBounded> mode{{pa, make_canvas(pa.d)}, aa,      pa.c[0], pa.c[1], pa.formula, pa.degree, ship,
                                      pa.formula == 0 && pa.degree == 2 && !ship};
  if constexpr (kJulia) mode.plot.constant(pa.c[0], pa.c[1]);
  run_rounds(pa.d, mode);
}

namespace {

typedef void (*AimKernel)(AimArgs);

// The aimed draws of one step, [bounded][fixed c], and every one there is, by step (draw_plot.h, plot_step_index).
struct AimStepKernels {
  AimKernel by[2][2];
};
#define CB_ROW(Step)                                                                \
  {{{draw_aim_kernel<Step, false, false>, draw_aim_kernel<Step, true, false>},      \
    {draw_aim_kernel<Step, false, true>, draw_aim_kernel<Step, true, true>}}},
constexpr AimStepKernels kAimKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kAimKernels) / sizeof(kAimKernels[0]) == kPlotSteps, "one row per step");

constexpr AimKernel kAimProbeKernels[2][2] = {{draw_aim_probe_kernel<false, false>, draw_aim_probe_kernel<true, false>},
                                              {draw_aim_probe_kernel<false, true>, draw_aim_probe_kernel<true, true>}};

}  // namespace

hipError_t launch_draw_aim(const AimArgs &a, bool lockstep, hipStream_t stream) {
  if (!plot_launch_ok(a.p) || a.p.palette != 0 || a.p.lut != nullptr) return hipErrorInvalidValue;
  if (!grid_launch_ok(a)) return hipErrorInvalidValue;
  if (a.p.d.n_threads == 0 || a.p.d.samples_per_thread == 0) return hipSuccess;
  const bool julia = a.p.julia != 0, bounded = a.bounded != 0, to_mask = a.mask != nullptr;
  const AimKernel kernel = lockstep  ? draw_aim_simple_kernel
                           : to_mask ? kAimProbeKernels[bounded][julia]
                                     : kAimKernels[plot_step_index(a.p)].by[bounded][julia];
  hipLaunchKernelGGL(kernel, dim3((a.p.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
