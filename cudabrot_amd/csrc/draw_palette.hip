// draw_palette.hip -- the palette render (include/cudabrot_amd.h, "Palette render"): a projected render or
// a Julia render whose accepted orbits are coloured by their escape index k.  lut[k] carries three integer weights, R in
// bits 0-7, G in bits 8-15, B in bits 16-23, and every in-canvas point of the orbit adds weight_j to its pixel in plane j
// of a histogram of three planes (plane_pixels apart), for every j with a non-zero weight.  Sample stream, rejection,
// interior map, iteration, escape index, accept filter, replayed points, projection and binning are the projected
// render's (a sampled c) or the Julia render's (a fixed one), unchanged.
//
// Kernels
//   draw_palette_simple_kernel      the definition verbatim, one lane per reference thread in lock-step, no early-out;
//                                   step, degree and Julia-or-not are run-time arguments.  Validation baseline
//                                   (cb_debug_last_draw_kernel 15).
//   draw_palette_kernel<Step, kJulia>  the product kernel (14): the round scheduler of draw_rounds.h with the palette plot
//                                   mode, one instance per step and per source of c.  An accepted orbit whose entry is
//                                   zero adds nothing anywhere, so it is not replayed: its steps go to skipped_steps.
//                                   Same histogram, generator states and counters (but skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_plot.h"

namespace cb {

namespace {

// One step with c = (c_re, c_im); degree 2 is the reference's step or its Burning Ship variant, else the Multibrot step.
__device__ __forceinline__ double palette_step(int degree, bool ship, double c_re, double c_im, double &r, double &i) {
  if (degree != 2) return power_step(degree, c_re, c_im, r, i);
  return ship ? mandel_step_ship(c_re, c_im, r, i) : mandel_step(c_re, c_im, r, i);
}

// The kernel's arguments read afresh, as draw_common.h's fresh_args reads a DrawArgs: what an accepted orbit alone needs
// (the table, c's columns of the matrix) is loaded where it is used and holds no scalar register across the loops.
typedef const PaletteArgs __attribute__((address_space(4))) *PaletteKernelArgs;
__device__ __forceinline__ PaletteKernelArgs fresh_palette_args() {
  PaletteKernelArgs p = (PaletteKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_palette_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_palette_simple_kernel(PaletteArgs pl) {
  const ProjectArgs &pa = pl.ja.pa;
  const DrawArgs &a = pa.d;
  const int d = pa.degree;
  const bool ship = a.burning_ship != 0;
  const bool julia = pl.julia != 0;
  const bool rejects = !julia && d == 2 && !ship;  // the Mandelbrot step on a sampled c: cardioid and bulb
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
      if (rejects && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      int k = a.max_iter;  // the first z_{k+1} that escapes; z_0 is not tested
      {
        double r = real, i = imag;
        for (int it = 0; it < a.max_iter; ++it) {
          if (palette_step(d, ship, c_re, c_im, r, i) > 4.0) {
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
      const PaletteKernelArgs now = fresh_palette_args();
      const uint32_t entry = now->lut[k];  // min_iter <= k < max_iter == n_entries, and 0 <= k
      const double ku = project_constant(now->ja.pa.p[2], now->ja.pa.p[3], c_re, c_im);
      const double kv = project_constant(now->ja.pa.p[6], now->ja.pa.p[7], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = palette_step(d, ship, c_re, c_im, r, i);
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
// draw_palette_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with PaletteMode of draw_plot.h, which is PlotMode (a sampled c) or JuliaMode (a
// fixed one) with another ESCAPED and another plot: step, NEXT and the never-escaping case are theirs.  ESCAPED counts
// the orbit as they do and then loads its entry, once: the lane keeps it through the replay.  A zero entry ends the
// sample there -- counted as recorded and in replay_steps like any accepted orbit, the replay not made in
// skipped_steps.  A replayed point finds its pixel once and adds each non-zero weight to that pixel of its plane.

template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_palette_kernel(PaletteArgs pl) {
  const ProjectArgs &pa = pl.ja.pa;
  if constexpr (kJulia) {
    // the plot's constant is made from the fixed c once, before the first round
    const double ku = project_constant(pa.p[2], pa.p[3], pl.ja.c[0], pl.ja.c[1]);
    const double kv = project_constant(pa.p[6], pa.p[7], pl.ja.c[0], pl.ja.c[1]);
    PaletteMode<Step, true> mode{{{pa, make_canvas(pa.d), ku, kv}, pl.ja.c[0], pl.ja.c[1]}, pl.lut, pl.plane_pixels};
    run_rounds(pa.d, mode);
  } else {
    PaletteMode<Step, false> mode{{{pa, make_canvas(pa.d)}}, pl.lut, pl.plane_pixels};
    run_rounds(pa.d, mode);
  }
}

namespace {

template <class Step>
void (*palette_kernel(bool julia))(PaletteArgs) {
  return julia ? draw_palette_kernel<Step, true> : draw_palette_kernel<Step, false>;
}

}  // namespace

hipError_t launch_draw_palette(const PaletteArgs &a, bool lockstep, hipStream_t stream) {
  const ProjectArgs &pa = a.ja.pa;
  const bool power = pa.degree != 2;
  const bool julia = a.julia != 0;
  if (power && (pa.degree < CB_POWER_MIN || pa.degree > CB_POWER_MAX || pa.d.burning_ship)) return hipErrorInvalidValue;
  for (int j = 0; julia && j < 2; ++j) {
    if (!(a.ja.c[j] >= -2.0 && a.ja.c[j] <= 2.0)) return hipErrorInvalidValue;  // a NaN fails both comparisons
  }
  // every accepted k indexes the table: the table covers [0, max_iter)
  if (a.lut == nullptr || pa.d.max_iter < 1 || pa.d.max_iter > CB_PALETTE_MAX_ENTRIES) return hipErrorInvalidValue;
  if (pa.d.n_threads == 0 || pa.d.samples_per_thread == 0) return hipSuccess;
  void (*kernel)(PaletteArgs) = nullptr;
  if (lockstep) {
    kernel = draw_palette_simple_kernel;
  } else {
    switch (pa.degree) {
      case 2:
        kernel = pa.d.burning_ship ? palette_kernel<ReferenceOrbit<true>>(julia) : palette_kernel<ReferenceOrbit<false>>(julia);
        break;
      case 3: kernel = palette_kernel<PowerOrbit<3>>(julia); break;
      case 4: kernel = palette_kernel<PowerOrbit<4>>(julia); break;
      case 5: kernel = palette_kernel<PowerOrbit<5>>(julia); break;
      case 6: kernel = palette_kernel<PowerOrbit<6>>(julia); break;
      case 7: kernel = palette_kernel<PowerOrbit<7>>(julia); break;
      default: kernel = palette_kernel<PowerOrbit<8>>(julia); break;
    }
  }
  hipLaunchKernelGGL(kernel, dim3((pa.d.n_threads + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace cb
