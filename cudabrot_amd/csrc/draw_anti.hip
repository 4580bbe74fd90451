// draw_anti.hip -- the anti-Buddhabrot (CB_KERNEL_FLAG_ANTI, include/cudabrot_amd.h): the orbits of the samples that do
// NOT escape, z_1 .. z_M, each binned as IncrementPixelCounter does (cudabrot.cu:302-314).
//
// Kernels (each for the Mandelbrot and the Burning Ship step)
//   draw_anti_simple_kernel  the naive definition, one lane per reference thread in lock-step: iterate to M, then
//                            replay all M points with weight 1.  Validation baseline (cb_debug_last_draw_kernel 5).
//   draw_anti_kernel         the product kernel (4): the same histogram and counters (but skipped_steps) with cycle
//                            compression: an orbit whose z is bit for bit a point it held at an earlier chunk boundary
//                            is replayed as its transient plus ONE period, each cycle point with its exact integer
//                            weight.  Lanes are refilled from their own subsequence every kAntiRound steps (DESIGN.md
//                            4.9), so that long, divergent transients do not idle the wave.
//
// Both add to the histogram with device-scope atomics (no workspace, no carry: every launch is complete).
#include "draw_common.h"

namespace cb {

namespace {

// kernels.hip's per-lane counters, summed over the wave at kernel end (one atomic per counter per wave); `reserved` is
// cb_counters.skipped_steps.
struct LaneStats {
  unsigned long long samples = 0, rejected = 0, never_escaped = 0, too_fast = 0, recorded = 0,
                     iterate_steps = 0, replay_steps = 0, increments = 0, reserved = 0,
                     status = 0;
};

__device__ __forceinline__ void flush_stats(cb_counters *counters, const LaneStats &s) {
  if (!counters) return;
  const unsigned long long v[10] = {
      wave_sum(s.samples),       wave_sum(s.rejected),     wave_sum(s.never_escaped),
      wave_sum(s.too_fast),      wave_sum(s.recorded),     wave_sum(s.iterate_steps),
      wave_sum(s.replay_steps),  wave_sum(s.increments),   wave_sum(s.reserved),
      wave_sum(s.status)};
  if (lane_id() == 0) {
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counters);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (v[i]) __hip_atomic_fetch_add(c + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (v[9]) __hip_atomic_fetch_or(c + 9, v[9], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool kShip>
__device__ __forceinline__ double anti_step(double cr, double ci, double &r, double &i) {
  return kShip ? mandel_step_ship(cr, ci, r, i) : mandel_step(cr, ci, r, i);
}

// Bit-for-bit equality of two points (not ==: -0.0 == 0.0, and a NaN equals nothing).
__device__ __forceinline__ bool same_bits(double r, double i, double sr, double si) {
  return __double_as_longlong(r) == __double_as_longlong(sr) && __double_as_longlong(i) == __double_as_longlong(si);
}

// Brent's schedule refined (draw_wave.hip long_retire): the saved point is replaced when the number of
// chunks done has no set bit below its top two -- after 1, 2, 3, 4, 6, 8, 12, 16, 24 ... chunks.
__device__ __forceinline__ bool brent_save(uint32_t chunks) {
  const int top = 31 - __clz((int) chunks);
  return top < 1 || (chunks & ((1u << (top - 1)) - 1u)) == 0u;
}

}  // namespace

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
      double r = real, i = imag;
      int k = max_iter;
      for (int it = 0; it < max_iter; ++it) {
        if ((a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i)) > 4.0) {
          k = it;
          break;
        }
      }
      if (k < max_iter) {  // escaped at z_{k+1}: nothing recorded
        st.too_fast++;
        st.iterate_steps += (unsigned long long) k + 1ull;
        continue;
      }
      st.never_escaped++;
      st.recorded++;
      st.iterate_steps += (unsigned long long) max_iter;
      r = real;
      i = imag;
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
// Every lane owns one reference thread (its generator, its samples_per_thread samples) and works on one sample at a
// time.  The wave advances in ROUNDS of kAntiRound steps; in a round each lane makes up to kAntiRound steps of its own
// phase, and between rounds each lane, on its own, does its bookkeeping:
//   ITERATE  z_k -> z_{k+kAntiRound} (fewer at M), testing |z|^2 > 4 after every step.  An escaping sample is done.
//            At k a multiple of kChunk: z_k == saved z_s bit for bit -> the orbit is the exact cycle z_s .. z_{k-1}
//            repeated (s >= kChunk > 0, k <= M: the definition's compression), start REPLAY with s and p = k - s;
//            else Brent's save.  At k == M without a match: REPLAY of all M points with weight 1.
//   REPLAY   z_j for j = 1 .. s - 1 + p from z_0 = c, the same steps: z_j, j < s, weight 1; the cycle point
//            z_{s+t}, 0 <= t < p, weight floor((M - s - t) / p) + 1 = q + 1 for t <= rem, q above, with
//            M - s = q p + rem.  Weights sum to (s - 1) + (M - s + 1) = M.
//   NEXT     draw the next sample of the lane's subsequence, or finish.
// A lane that completes a phase mid-round idles to the round's end: kAntiRound steps are the grain of the refill.
// Rounds divide kChunk, so an iterating lane is at a chunk boundary exactly when k % kChunk == 0.
constexpr int kAntiRound = 12;
static_assert(kChunk % kAntiRound == 0, "an iterating lane meets every chunk boundary at a round's end");

enum : int { kAntiNext = 0, kAntiIterate = 1, kAntiReplay = 2, kAntiDone = 3 };

template <bool kShip>
__global__ void __launch_bounds__(256) draw_anti_kernel(DrawArgs a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter > 0 ? a.max_iter : 0;
  LaneStats st;
  Xorwow rng = {0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) rng = load_rng(a.states, a.n_threads, tid);
  uint32_t left = valid ? a.samples_per_thread : 0u;
  int phase = kAntiNext;
  double cr = 0.0, ci = 0.0, r = 0.0, i = 0.0;  // the sample and its orbit: z_k
  double sr = 0.0, si = 0.0;                      // ITERATE: the saved point z_saved
  int k = 0;                                      // index of z
  int saved = 0;                                  // ITERATE: index of the saved point (0: none yet)
  int end = 0;                                    // REPLAY: last index replayed (s - 1 + p)
  int cyc = 0;                                    // REPLAY: s, the first cycle point (> max_iter: no cycle)
  int rem = 0;                                    // REPLAY: weight q + 1 up to z_{s+rem}, q after it
  unsigned long long q = 0ull;
  while (true) {
    // ---- between rounds: each lane's bookkeeping --------------------------------------------------------------
    if (phase == kAntiNext) {
      while (left > 0u) {
        left--;
        cr = sample_coordinate(rng);
        ci = sample_coordinate(rng);
        st.samples++;
        if (max_iter == 0) {  // nothing to test, nothing to record
          st.never_escaped++;
          st.recorded++;
          continue;
        }
        r = cr;
        i = ci;
        k = 0;
        saved = 0;
        phase = kAntiIterate;
        break;
      }
      if (phase == kAntiNext) phase = kAntiDone;
    }
    if (__ballot(phase != kAntiDone) == 0ull) break;
    // ---- one round ----------------------------------------------------------------------------------------------
    const int limit = phase == kAntiIterate ? max_iter : end;
    const int stop = phase == kAntiDone ? k : (limit - k < kAntiRound ? limit : k + kAntiRound);
#pragma unroll 2
    for (int t = 0; t < kAntiRound; ++t) {
      if (k < stop) {
        const double m = anti_step<kShip>(cr, ci, r, i);
        ++k;
        if (phase == kAntiReplay) {
          int row, col;
          if (pixel_of(r, i, cv, row, col)) {
            const unsigned long long w = k < cyc ? 1ull : (k - cyc <= rem ? q + 1ull : q);
            add_to_pixel(a.hist, cv, row, col, w);
            st.increments += w;
          }
        } else if (m > 4.0) {  // escaped at z_k: nothing recorded
          st.too_fast++;
          st.iterate_steps += (unsigned long long) k;
          phase = kAntiNext;
          k = stop;  // no more steps this round
        }
      }
    }
    if (phase == kAntiReplay) {
      if (k == end) phase = kAntiNext;
    } else if (phase == kAntiIterate) {
      bool start = false;
      const bool boundary = (k % kChunk) == 0;
      if (boundary && saved > 0 && same_bits(r, i, sr, si)) {
        // z_k == z_saved: the exact cycle z_saved .. z_{k-1}, p = k - saved (a multiple of the least period)
        const int p = k - saved;
        cyc = saved;
        end = saved - 1 + p;
        q = (unsigned long long) ((max_iter - saved) / p);
        rem = (max_iter - saved) % p;
        st.reserved += (unsigned long long) (max_iter - k) + (unsigned long long) (max_iter - end);
        start = true;
      } else if (k == max_iter) {
        cyc = max_iter + 1;  // no cycle seen: all M points with weight 1
        end = max_iter;
        q = 0ull;
        rem = 0;
        start = true;
      } else if (boundary && brent_save((uint32_t) (k / kChunk))) {
        sr = r;
        si = i;
        saved = k;
      }
      if (start) {
        st.never_escaped++;
        st.recorded++;
        st.iterate_steps += (unsigned long long) max_iter;
        st.replay_steps += (unsigned long long) max_iter;
        r = cr;
        i = ci;
        k = 0;
        phase = kAntiReplay;
      }
    }
  }
  if (valid) store_rng(a.states, a.n_threads, tid, rng);
  flush_stats(a.counters, st);
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
