// draw_anti.hip -- the anti-Buddhabrot (CB_KERNEL_FLAG_ANTI, include/cudabrot_amd.h): the orbits of the samples that do
// NOT escape, z_1 .. z_M, each binned as IncrementPixelCounter does (cudabrot.cu:302-314).
//
// Kernels (each for the Mandelbrot and the Burning Ship step)
//   draw_anti_simple_kernel  the naive definition, one lane per reference thread in lock-step: iterate to M, then
//                            replay all M points with weight 1.  Validation baseline (cb_debug_last_draw_kernel 5).
//   draw_anti_kernel         the product kernel (4): the same histogram and counters (but skipped_steps) with cycle
//                            compression: an orbit whose z is bit for bit a point it held at an earlier chunk boundary
//                            is replayed as its transient plus ONE period, each cycle point with its exact integer
//                            weight.  Lanes are refilled from their own subsequence every kRound steps (draw_rounds.h,
//                            DESIGN.md 4.9), so that long, divergent transients do not idle the wave.
//
// Both add to the histogram with device-scope atomics (no workspace, no carry: every launch is complete).
#include "draw_rounds.h"

namespace cb {

// ------------------------------------------------------------------------------------------------
// draw_anti_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_anti_simple_kernel(DrawArgs a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter > 0 ? a.max_iter : 0;
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);
      const double imag = sample_coordinate(rng);
      st.samples++;
      const int k = escape_index(real, imag, max_iter, a.burning_ship);
      if (k < max_iter) {  // escaped at z_{k+1}: nothing recorded
        st.too_fast++;
        st.iterate_steps += (unsigned long long) k + 1ull;
        continue;
      }
      st.never_escaped++;
      st.recorded++;
      st.iterate_steps += (unsigned long long) max_iter;
      double r = real, i = imag;
      for (int it = 0; it < max_iter; ++it) {
        (void) (a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i));
        st.replay_steps++;
        st.increments += increment_pixel_counter(r, i, a.hist, cv) ? 1ull : 0ull;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_anti_kernel: cycle-compressed, lanes refilled from their own subsequence
// ------------------------------------------------------------------------------------------------
//
// The round scheduler of draw_rounds.h with this mode: no sample is rejected, an escaping one records nothing, and a
// sample that does not escape is replayed.
//   cycle z_s .. z_{k-1} found (s = saved >= kChunk > 0, k <= M, p = k - s: the definition's compression): REPLAY of
//            z_j for j = 1 .. s - 1 + p: z_j, j < s, weight 1; the cycle point z_{s+t}, 0 <= t < p, weight
//            floor((M - s - t) / p) + 1 = q + 1 for t <= rem, q above, with M - s = q p + rem.  Weights sum to
//            (s - 1) + (M - s + 1) = M.
//   k == M without a match: REPLAY of all M points with weight 1.

namespace {

template <bool kShipStep>
struct AntiMode {
  static constexpr bool kShip = kShipStep;
  const DrawArgs &a;
  const Canvas cv;
  int cyc = 0;  // REPLAY: s, the first cycle point (> max_iter: no cycle)
  int rem = 0;  // REPLAY: weight q + 1 up to z_{s+rem}, q after it
  unsigned long long q = 0ull;

  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) {
    uniform_sample(rng, l.cr, l.ci);
    return kSampleIterate;
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
    return true;
  }

  __device__ __forceinline__ bool point(RoundLane &l, LaneStats &st) {
    int row, col;
    if (pixel_of(l.r, l.i, cv, row, col)) {
      const unsigned long long w = l.k < cyc ? 1ull : (l.k - cyc <= rem ? q + 1ull : q);
      add_to_pixel(a.hist, cv, row, col, w);
      st.increments += w;
    }
    return false;
  }
};

}  // namespace

template <bool kShip>
__global__ void __launch_bounds__(256) draw_anti_kernel(DrawArgs a) {
  AntiMode<kShip> mode{a, make_canvas(a)};
  run_rounds(a, mode);
}

hipError_t launch_draw_anti(const DrawArgs &a, bool lockstep, hipStream_t stream) {
  if (a.n_threads == 0 || a.samples_per_thread == 0) return hipSuccess;
  const uint32_t blocks = (a.n_threads + 255u) / 256u;
  if (lockstep) {
    hipLaunchKernelGGL(draw_anti_simple_kernel, dim3(blocks), dim3(256), 0, stream, a);
  } else if (a.burning_ship) {
    hipLaunchKernelGGL(draw_anti_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(draw_anti_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace cb
