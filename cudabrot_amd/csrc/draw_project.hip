// draw_project.hip -- the projected render (include/cudabrot_amd.h, "Projected render"): every recorded
// orbit point is a point (z_re, z_im, c_re, c_im) of a four-dimensional set, and a 2 x 4 matrix P picks the plane it is
// plotted on:
//   K_u = fma(P[0][2], c_re, P[0][3] * c_im)             (once per sample)
//   u   = fma(P[0][0], z_re, fma(P[0][1], z_im, K_u))
// and v likewise from row 1; (u, v) is binned as the reference bins (re, im).  Samples, cardioid / bulb rejection (not
// for the Burning Ship), IterateMandelbrot, the accept filter min <= k < max and the replayed points z_1 .. z_{k+1} are
// the normal render's.
//
// Kernels
//   draw_project_simple_kernel  the definition verbatim, one lane per reference thread in lock-step, no early-out; the
//                               step is a run-time switch.  Validation baseline (cb_debug_last_draw_kernel 9).
//   draw_project_kernel         the product kernel (8), a template over the step: lanes are refilled from their own
//                               subsequence every kProjectRound steps (draw_focus.hip's scheduling), a new sample is
//                               looked up in the interior map (Mandelbrot step only) and a marked one retired without
//                               iterating, and an orbit found exactly periodic at a chunk boundary is
//                               retired as never-escaping.  Same histogram, generator states and counters (but
//                               skipped_steps).
// No workspace, no carry, no LDS: every launch is complete, and lane t advances generator t by exactly its samples.
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
__device__ __forceinline__ double project_step(double cr, double ci, double &r, double &i) {
  return kShip ? mandel_step_ship(cr, ci, r, i) : mandel_step(cr, ci, r, i);
}

// Bit-for-bit equality of two points (not ==: -0.0 == 0.0, and a NaN equals nothing).
__device__ __forceinline__ bool same_bits(double r, double i, double sr, double si) {
  return __double_as_longlong(r) == __double_as_longlong(sr) && __double_as_longlong(i) == __double_as_longlong(si);
}

// Brent's schedule refined: the saved point is replaced after 1, 2, 3, 4, 6, 8, 12, 16, 24 ... chunks.
__device__ __forceinline__ bool brent_save(uint32_t chunks) {
  const int top = 31 - __clz((int) chunks);
  return top < 1 || (chunks & ((1u << (top - 1)) - 1u)) == 0u;
}

// The sample's part of a plotted coordinate: the two columns of P that multiply c.
__device__ __forceinline__ double project_constant(double pc_re, double pc_im, double cr, double ci) {
  return __builtin_fma(pc_re, cr, pc_im * ci);
}
// One plotted coordinate of the point (r, i): the two columns of P that multiply z, and the sample's constant.
__device__ __forceinline__ double project_point(double pz_re, double pz_im, double r, double i, double k) {
  return __builtin_fma(pz_re, r, __builtin_fma(pz_im, i, k));
}

// The interior map (DrawArgs::interior_map), on undoubled coordinates: column floor((c_re + 2) 2^level), row
// floor(|c_im| 2^level), level = interior_shift + 1; c_re + 2 is exact for every sample of the stream.  true: every
// sample of the cell that holds c provably never escapes.
__device__ __forceinline__ bool interior_marked(const DrawArgs &a, double cr, double ci) {
  const int level = (int) a.interior_shift + 1;
  const double x = __builtin_ldexp(cr + 2.0, level);
  const double y = __builtin_ldexp(__builtin_fabs(ci), level);
  if (!(x >= 0.0)) return false;
  const uint32_t col = (uint32_t) x;
  const uint32_t row = (uint32_t) y;
  if (col >= a.interior_cols || row >= a.interior_rows) return false;
  const uint32_t index = row * a.interior_cols + col;  // < 2.5 * 1.25 * 4^level
  return ((a.interior_map[index >> 3] >> (index & 7u)) & 1u) != 0u;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_project_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_project_simple_kernel(ProjectArgs pa) {
  const DrawArgs &a = pa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      const double real = sample_coordinate(rng);
      const double imag = sample_coordinate(rng);
      st.samples++;
      if (!a.burning_ship && (in_main_cardioid(real, imag) || in_order2_bulb(real, imag))) {
        st.rejected++;
        continue;
      }
      double r = real, i = imag;
      int k = a.max_iter;
      for (int it = 0; it < a.max_iter; ++it) {
        if ((a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i)) > 4.0) {
          k = it;
          break;
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
      const double ku = project_constant(pa.p[2], pa.p[3], real, imag);
      const double kv = project_constant(pa.p[6], pa.p[7], real, imag);
      r = real;
      i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i);
        st.replay_steps++;
        const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
        const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
        int row, col;
        if (pixel_of(u, v, cv, row, col)) {
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
// draw_project_kernel: lanes refilled from their own subsequence, interior map, exact-periodicity early-out
// ------------------------------------------------------------------------------------------------
//
// Every lane owns one reference thread (its generator, its samples_per_thread samples) and works on one sample at a
// time.  The wave advances in ROUNDS of kProjectRound steps; in a round each lane makes up to kProjectRound steps of its
// own phase, and between rounds each lane, on its own, does its bookkeeping:
//   NEXT     draw the lane's next sample (rejecting cardioid and bulb) and look it up in the interior map (Mandelbrot
//            step only): a marked one is retired as the reference counts it (never_escaped, max_iter iterate steps), all
//            of them in skipped_steps.  The first sample that is neither goes to ITERATE.  Or finish.  (A short run of
//            tested steps inside this loop, for the 91 % of uniform samples that escape within four, was built and
//            measured: slower)
//   ITERATE  z_k -> z_{k+kProjectRound} (fewer at max_iter), testing |z|^2 > 4 after every step.  A lane that escapes at
//            its n-th step (the reference's k = n - 1) notes n and idles to the round's end (ESCAPED); there the accept
//            filter sends it to NEXT (too fast) or REPLAY.  At k a multiple of kChunk: z_k == the saved point bit for
//            bit -> the orbit is an exact cycle of points that all passed the test, so it never escapes: counted as the
//            reference counts it, the steps not made in skipped_steps; else Brent's save.  At k == max_iter: never
//            escaped.
//   REPLAY   z_1 .. z_n from z_0 = c, the same steps bit for bit, so the n-th is the one that escapes: each projected
//            and binned (device-scope atomics).
// Rounds divide kChunk, so an iterating lane is at a chunk boundary exactly when k % kChunk == 0.
constexpr int kProjectRound = 12;
static_assert(kChunk % kProjectRound == 0, "an iterating lane meets every chunk boundary at a round's end");

enum : int { kProjectNext = 0, kProjectIterate = 1, kProjectReplay = 2, kProjectEscaped = 3, kProjectDone = 4 };

template <bool kShip>
__global__ void __launch_bounds__(256) draw_project_kernel(ProjectArgs pa) {
  const DrawArgs &a = pa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter;
  const bool use_map = !kShip && a.interior_map != nullptr;
  LaneStats st;
  Xorwow rng = {0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) rng = load_rng(a.states, a.n_threads, tid);
  uint32_t left = valid ? a.samples_per_thread : 0u;
  int phase = kProjectNext;
  double cr = 0.0, ci = 0.0, r = 0.0, i = 0.0;  // the sample and its orbit: z_k
  double sr = 0.0, si = 0.0;                      // ITERATE: the saved point
  double ku = 0.0, kv = 0.0;                      // REPLAY: the sample's part of (u, v)
  int k = 0;                                      // index of z
  int saved = 0;                                  // ITERATE: index of the saved point (0: none yet)
  int end = 0;                                    // ESCAPED, REPLAY: the step that escapes
  while (true) {
    // ---- between rounds: each lane's bookkeeping --------------------------------------------------------------
    if (phase == kProjectNext) {
      while (left > 0u) {
        left--;
        cr = sample_coordinate(rng);
        ci = sample_coordinate(rng);
        st.samples++;
        if (!kShip && (in_main_cardioid(cr, ci) || in_order2_bulb(cr, ci))) {
          st.rejected++;
          continue;
        }
        if (max_iter <= 0) {  // IterateMandelbrot returns max at once
          st.never_escaped++;
          continue;
        }
        if (use_map && interior_marked(a, cr, ci)) {  // retired without iterating
          st.never_escaped++;
          st.iterate_steps += (unsigned long long) max_iter;
          st.reserved += (unsigned long long) max_iter;
          continue;
        }
        r = cr;
        i = ci;
        k = 0;
        saved = 0;
        phase = kProjectIterate;
        break;
      }
      if (phase == kProjectNext) phase = kProjectDone;
    }
    if (__ballot(phase != kProjectDone) == 0ull) break;
    // ---- one round ----------------------------------------------------------------------------------------------
    const int limit = phase == kProjectIterate ? max_iter : end;
    const int stop = phase == kProjectDone ? k : (limit - k < kProjectRound ? limit : k + kProjectRound);
#pragma unroll 2
    for (int t = 0; t < kProjectRound; ++t) {
      if (k < stop) {
        const double m = project_step<kShip>(cr, ci, r, i);
        ++k;
        if (phase == kProjectReplay) {
          const double u = project_point(pa.p[0], pa.p[1], r, i, ku);
          const double v = project_point(pa.p[4], pa.p[5], r, i, kv);
          int row, col;
          if (pixel_of(u, v, cv, row, col)) {
            add_to_pixel(a.hist, cv, row, col, 1ull);
            st.increments++;
          }
        } else if (m > 4.0) {  // escaped at z_k
          end = k;
          phase = kProjectEscaped;
          k = stop;  // no more steps this round
        }
      }
    }
    if (phase == kProjectReplay) {
      if (k == end) phase = kProjectNext;
    } else if (phase == kProjectEscaped) {
      st.iterate_steps += (unsigned long long) end;
      if (end - 1 < a.min_iter) {
        st.too_fast++;
        phase = kProjectNext;
      } else {
        st.recorded++;
        st.replay_steps += (unsigned long long) end;
        ku = project_constant(pa.p[2], pa.p[3], cr, ci);
        kv = project_constant(pa.p[6], pa.p[7], cr, ci);
        r = cr;
        i = ci;
        k = 0;
        phase = kProjectReplay;
      }
    } else if (phase == kProjectIterate) {
      const bool boundary = (k % kChunk) == 0;
      if (k == max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) max_iter;
        phase = kProjectNext;
      } else if (boundary && saved > 0 && same_bits(r, i, sr, si)) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) max_iter;
        st.reserved += (unsigned long long) (max_iter - k);
        phase = kProjectNext;
      } else if (boundary && brent_save((uint32_t) (k / kChunk))) {
        sr = r;
        si = i;
        saved = k;
      }
    }
  }
  if (valid) store_rng(a.states, a.n_threads, tid, rng);
  flush_stats(a.counters, st);
}

hipError_t launch_draw_project(const ProjectArgs &a, bool lockstep, hipStream_t stream) {
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const uint32_t blocks = (a.d.n_threads + 255u) / 256u;
  if (lockstep) {
    hipLaunchKernelGGL(draw_project_simple_kernel, dim3(blocks), dim3(256), 0, stream, a);
  } else if (a.d.burning_ship) {
    hipLaunchKernelGGL(draw_project_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(draw_project_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace cb
