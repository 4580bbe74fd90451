// draw_depth_palette.hip -- the depth-palette render (include/cudabrot_amd.h, "Depth-palette render"): a
// depth render (draw_depth.hip) whose slice s is not a plane but the index of a colour.  A visited point that is on the
// canvas and in depth adds weight_j(lut[s]) to its pixel of plane j of THREE planes, for every j with a non-zero weight:
// the palette render's sink (draw_plot.h, PaletteMode) keyed by depth instead of escape index.  Everything before the add
// -- sample stream, rejection, interior map, iteration, accept filter, replayed points, (u, v), d and the slice -- is the
// depth render's, and so is every counter but increments, which is the sum of the weights added.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_depth_palette_simple_kernel        the definition verbatim, one lane per reference thread in lock-step, no
//                                           early-out; the table is read from global memory at every point.  Validation
//                                           baseline (21).
//   draw_depth_palette_kernel<Step, kJulia> the product kernel (20): the round scheduler of draw_rounds.h with
//                                           DepthPaletteMode, which is DepthMode (draw_depth.h) with another plot.  One
//                                           instance per step (13) and per source of c (2): 26.
// The table.  The palette render looks its entry up once per orbit; here the lookup is once per plotted point, a divergent
// 4-byte gather.  The product kernel stages the table -- at most CB_DEPTH_MAX_SLICES = 256 entries, 1 KiB -- in static LDS
// at kernel start: thread t of the 256 loads entry t if there is one, then one barrier before the first round.  1 KiB per
// workgroup costs no occupancy, and the lookup is a ds_read_b32 that does not queue behind the atomics in the vector
// memory pipeline.  No workspace, no carry: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_depth.h"

namespace cb {

namespace {

typedef const DepthPaletteArgs __attribute__((address_space(4))) *DepthPaletteKernelArgs;
__device__ __forceinline__ DepthPaletteKernelArgs fresh_depth_palette_args() {
  DepthPaletteKernelArgs p = (DepthPaletteKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// What a point on the canvas and in depth adds: each non-zero weight of its slice's entry to its pixel of that plane.
__device__ __forceinline__ void add_entry(unsigned long long *hist, unsigned long long plane_pixels, const Canvas &cv,
                                          int row, int col, uint32_t entry, LaneStats &st) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned long long weight = palette_weight(entry, j);
    if (weight != 0ull) {
      add_to_pixel(hist + (unsigned long long) j * plane_pixels, cv, row, col, weight);
      st.increments += weight;
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The lock-step kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_depth_palette_simple_kernel(DepthPaletteArgs dpa) {
  const DepthArgs &da = dpa.d;
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
      const DepthPaletteKernelArgs now = fresh_depth_palette_args();
      const double ku = project_constant(now->d.p.p[2], now->d.p.p[3], c_re, c_im);
      const double kv = project_constant(now->d.p.p[6], now->d.p.p[7], c_re, c_im);
      const double kd = project_constant(now->d.row[2], now->d.row[3], c_re, c_im);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = depth_step(f, deg, ship, c_re, c_im, r, i);
        st.replay_steps++;
        const double u = project_point(now->d.p.p[0], now->d.p.p[1], r, i, ku);
        const double v = project_point(now->d.p.p[4], now->d.p.p[5], r, i, kv);
        const double d = project_point(now->d.row[0], now->d.row[1], r, i, kd);
        int row, col, s;
        if (pixel_of(u, v, cv, row, col) &&
            slice_of(d, now->d.min, now->d.delta, now->d.inv_delta, now->d.pow2, now->d.slices, s)) {
          // 0 <= s < slices == the table's entries
          add_entry(a.hist, now->plane_pixels, cv, row, col, now->lut[s] & kPaletteWeightBits, st);
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
// draw_depth_palette_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// DepthMode (draw_depth.h) with another plot: step, NEXT, ESCAPED (which makes K_d of a sampled c) and the never-escaping
// case are DepthMode's; a replayed point finds its pixel and its slice as there, reads the slice's entry from the staged
// table and makes up to three adds.  The body stands in the kernel, not in a function the kernel calls.

namespace {

template <class Step, bool kJulia>
struct DepthPaletteMode {
  DepthMode<Step, kJulia> depth;
  const uint32_t *const table;  // the workgroup's copy, in LDS: da.slices entries
  const unsigned long long plane_pixels;

  __device__ __forceinline__ double step(RoundLane &l) { return depth.step(l); }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) { return depth.next(rng, l); }
  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) { return depth.escaped(l, st); }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    return depth.never_escapes(l, st, cycle);
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    const Plot &plot = depth.base.plot;
    const DepthArgs &da = depth.da;
    const double u = project_point(plot.pa.p[0], plot.pa.p[1], l.r, l.i, plot.ku);
    const double v = project_point(plot.pa.p[4], plot.pa.p[5], l.r, l.i, plot.kv);
    const double d = project_point(da.row[0], da.row[1], l.r, l.i, depth.kd);
    int row, col, s;
    if (pixel_of(u, v, plot.cv, row, col) && slice_of(d, da.min, da.delta, da.inv_delta, da.pow2, da.slices, s)) {
      add_entry(plot.pa.d.hist, plane_pixels, plot.cv, row, col, table[s], st);  // 0 <= s < slices <= 256
    }
    return false;
  }
};

}  // namespace

template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_depth_palette_kernel(DepthPaletteArgs dpa) {
  // Every thread of the workgroup takes part, the lanes past n_threads too: the barrier is met by all 256 before any of
  // them can leave, and run_rounds has none.
  __shared__ uint32_t table[CB_DEPTH_MAX_SLICES];
  static_assert(CB_DEPTH_MAX_SLICES <= 256, "one entry per thread of the workgroup");
  if ((int) threadIdx.x < dpa.d.slices) table[threadIdx.x] = dpa.lut[threadIdx.x] & kPaletteWeightBits;
  __syncthreads();
  const DepthArgs &da = dpa.d;
  const PlotArgs &pa = da.p;
  if constexpr (kJulia) {
    const double ku = project_constant(pa.p[2], pa.p[3], pa.c[0], pa.c[1]);
    const double kv = project_constant(pa.p[6], pa.p[7], pa.c[0], pa.c[1]);
    const double kd = project_constant(da.row[2], da.row[3], pa.c[0], pa.c[1]);
    DepthPaletteMode<Step, true> mode{{{{pa, make_canvas(pa.d), ku, kv}, pa.c[0], pa.c[1]}, da, kd}, table, dpa.plane_pixels};
    run_rounds(pa.d, mode);
  } else {
    DepthPaletteMode<Step, false> mode{{{{pa, make_canvas(pa.d)}}, da}, table, dpa.plane_pixels};
    run_rounds(pa.d, mode);
  }
}

namespace {

typedef void (*DepthPaletteKernel)(DepthPaletteArgs);

// The product kernels of one step, [fixed c], and every one there is, by step (draw_plot.h, plot_step_index):
// draw_depth.hip's instance set.
struct StepKernels {
  DepthPaletteKernel by[2];
};
#define CB_ROW(Step) {{draw_depth_palette_kernel<Step, false>, draw_depth_palette_kernel<Step, true>}},
constexpr StepKernels kDepthPaletteKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kDepthPaletteKernels) / sizeof(kDepthPaletteKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_depth_palette(const DepthPaletteArgs &dpa, uint32_t n_entries, bool lockstep, hipStream_t stream) {
  const DepthArgs &da = dpa.d;
  const PlotArgs &a = da.p;
  if (!depth_launch_ok(da)) return hipErrorInvalidValue;
  if (a.palette != 0 || a.lut != nullptr) return hipErrorInvalidValue;  // the palette render's table has no place here
  // the table holds an entry for every slice the kernels can compute, and the three planes lie w * h apart
  if (dpa.lut == nullptr || n_entries != (uint32_t) da.slices || dpa.plane_pixels != da.plane_pixels) {
    return hipErrorInvalidValue;
  }
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const DepthPaletteKernel kernel =
      lockstep ? draw_depth_palette_simple_kernel : kDepthPaletteKernels[plot_step_index(a)].by[a.julia != 0];
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, dpa);
  return hipGetLastError();
}

}  // namespace cb
