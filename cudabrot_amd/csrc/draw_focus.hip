// draw_focus.hip -- the focused render (include/cudabrot_amd.h, "Focused render"): a cropped canvas
// sampled only from the cells of the c-plane whose samples reach it.
//
// One kernel over a SOURCE of samples and a SINK of accepted orbits (FocusArgs, kernels.h):
//   source  uniform   the normal stream: 4 XORWOW draws per sample, c uniform over [-2, 2)^2
//           cells     6 draws per sample: a cell of the list (two draws), a point of that cell (four)
//   sink    histogram every in-canvas point of the replay is added to the histogram (device-scope atomics)
//           mask      the probe: the replay stops at its first in-canvas point and sets the bit of the cell that holds c
// From c on everything is the reference's: cardioid / bulb rejection (not for the Burning Ship), IterateMandelbrot, the
// accept filter min <= k < max, IterateAndRecord.
//
// Kernels
//   draw_focus_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; source,
//                             sink and step are run-time switches.  Validation baseline (cb_debug_last_draw_kernel 7).
//   draw_focus_kernel         the product kernel (6), a template over source, sink and step: lanes are refilled from
//                             their own subsequence every kRound steps (draw_rounds.h), and an orbit found exactly periodic at a
//                             chunk boundary is retired as never-escaping.  Same histogram, mask,
//                             generator states and counters (but skipped_steps).
// No workspace, no carry: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_cells.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// draw_focus_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_focus_simple_kernel(FocusArgs fa) {
  const DrawArgs &a = fa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const bool from_cells = fa.g.cells != nullptr;
  const bool to_mask = fa.g.mask != nullptr;
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      double real, imag;
      if (from_cells) {
        next_sample<true>(fa.g, rng, real, imag);
      } else {
        next_sample<false>(fa.g, rng, real, imag);
      }
      st.samples++;
      if (!a.burning_ship && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      const int k = escape_index(real, imag, a.max_iter, a.burning_ship);
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
      if (!to_mask) st.recorded++;
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i);
        st.replay_steps++;
        int row, col;
        if (pixel_of(r, i, cv, row, col)) {
          if (to_mask) {  // the first in-canvas point: the sample's cell reaches the canvas
            mark_cell(fa.g, real, imag);
            st.recorded++;
            break;
          }
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

// ------------------------------------------------------------------------------------------------
// draw_focus_kernel: lanes refilled from their own subsequence, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode: NEXT draws from the source and rejects cardioid and bulb; an
// escape goes through the accept filter to REPLAY of z_1 .. z_n, the n-th being the one that escapes; an exact cycle
// never escapes and is counted as the reference counts it (never_escaped, max_iter iterate steps), the steps not made
// in skipped_steps.  The histogram sink adds every in-canvas point of the replay, the mask sink stops at the first.

namespace {

template <bool kCells, bool kMask, bool kShipStep>
struct FocusMode {
  static constexpr bool kShip = kShipStep;
  const FocusArgs &fa;
  const Canvas cv;

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    next_sample<kCells>(fa.g, rng, l.cr, l.ci);
    if (!kShip && (in_main_cardioid(l.cr, l.ci) || in_order2_bulb(l.cr, l.ci))) return kSampleRejected;
    return kSampleIterate;
  }

  // the mask sink counts `recorded` at the point that ends its replay, and gives back the steps it does not make
  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) {
    return count_escaped(l, fa.d.min_iter, st, !kMask);
  }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool) { return count_never_escapes(l, st); }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    int row, col;
    if (!pixel_of(l.r, l.i, cv, row, col)) return false;
    if (kMask) {  // the first in-canvas point ends the replay
      mark_cell(fa.g, l.cr, l.ci);
      st.recorded++;
      st.replay_steps -= (unsigned long long) (l.end - l.k);
      return true;
    }
    add_to_pixel(fa.d.hist, cv, row, col, 1ull);
    st.increments++;
    return false;
  }
};

}  // namespace

template <bool kCells, bool kMask, bool kShip>
__global__ void __launch_bounds__(256) draw_focus_kernel(FocusArgs fa) {
  FocusMode<kCells, kMask, kShip> mode{fa, make_canvas(fa.d)};
  run_rounds(fa.d, mode);
}

namespace {

template <bool kCells, bool kMask>
void launch_product(const FocusArgs &a, uint32_t blocks, hipStream_t stream) {
  if (a.d.burning_ship) {
    hipLaunchKernelGGL((draw_focus_kernel<kCells, kMask, true>), dim3(blocks), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL((draw_focus_kernel<kCells, kMask, false>), dim3(blocks), dim3(256), 0, stream, a);
  }
}

}  // namespace

hipError_t launch_draw_focus(const FocusArgs &a, bool lockstep, hipStream_t stream) {
  if (!grid_launch_ok(a.g)) return hipErrorInvalidValue;
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const uint32_t blocks = (a.d.n_threads + 255u) / 256u;
  const bool from_cells = a.g.cells != nullptr, to_mask = a.g.mask != nullptr;
  if (lockstep) {
    hipLaunchKernelGGL(draw_focus_simple_kernel, dim3(blocks), dim3(256), 0, stream, a);
  } else if (from_cells && !to_mask) {  // the focused draw
    launch_product<true, false>(a, blocks, stream);
  } else if (!from_cells && to_mask) {  // the probe
    launch_product<false, true>(a, blocks, stream);
  } else {  // a normal render through this kernel (the tests' check against the oracle)
    launch_product<false, false>(a, blocks, stream);
  }
  return hipGetLastError();
}

}  // namespace cb
