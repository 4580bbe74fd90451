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
//                             their own subsequence every kFocusRound steps, and an orbit found exactly periodic at a
//                             chunk boundary is retired as never-escaping.  Same histogram, mask,
//                             generator states and counters (but skipped_steps).
// No workspace, no carry: every launch is complete, and lane t advances generator t by exactly its samples.
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
__device__ __forceinline__ double focus_step(double cr, double ci, double &r, double &i) {
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

// The next sample of a thread.  Uniform source: two coordinates, two draws each.  Cell list: a, b -> entry
// j = high half of (a << 32 | b) * n_cells, then a point of that cell: the offset (x + 2) * 2^-(level + 2) is exact
// (x + 2 = (v + 1) * 2^-51, v < 2^53), the cell's corner is exact, so each coordinate is ONE rounded addition.
template <bool kCells>
__device__ __forceinline__ void next_sample(const FocusArgs &a, Xorwow &rng, double &cr, double &ci) {
  if (kCells) {
    const uint32_t hi = xorwow_next(rng);
    const uint32_t lo = xorwow_next(rng);
    const unsigned long long ab = ((unsigned long long) hi << 32) | (unsigned long long) lo;
    const uint32_t j = (uint32_t) __umul64hi(ab, (unsigned long long) a.n_cells);  // < n_cells
    const uint32_t cell = a.cells[j];
    const uint32_t shift = (uint32_t) a.level + 2u;  // n = 4 * 2^level cells per side
    const uint32_t col = cell & ((1u << shift) - 1u);
    const uint32_t row = cell >> shift;
    const double x = sample_coordinate(rng);
    const double y = sample_coordinate(rng);
    const double lo_re = -2.0 + (double) col * a.cell_side;
    const double lo_im = -2.0 + (double) row * a.cell_side;
    const double off_re = (x + 2.0) * a.cell_scale;
    const double off_im = (y + 2.0) * a.cell_scale;
    cr = lo_re + off_re;
    ci = lo_im + off_im;
  } else {
    cr = sample_coordinate(rng);
    ci = sample_coordinate(rng);
  }
}

// The probe's sink: the bit of the cell that holds c.  (c + 2) * 2^level is exact; c = 2 exactly, which
// sample_coordinate can return, is clamped into the last cell.
__device__ __forceinline__ void mark_cell(const FocusArgs &a, double cr, double ci) {
  const int n = 4 << a.level;
  int col = (int) ((cr + 2.0) * a.cells_per_unit);
  int row = (int) ((ci + 2.0) * a.cells_per_unit);
  col = col < 0 ? 0 : (col > n - 1 ? n - 1 : col);
  row = row < 0 ? 0 : (row > n - 1 ? n - 1 : row);
  const uint32_t index = (uint32_t) row * (uint32_t) n + (uint32_t) col;
  __hip_atomic_fetch_or(a.mask + (index >> 5), 1u << (index & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// draw_focus_simple_kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_focus_simple_kernel(FocusArgs fa) {
  const DrawArgs &a = fa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const bool from_cells = fa.cells != nullptr;
  const bool to_mask = fa.mask != nullptr;
  LaneStats st;
  if (valid) {
    Xorwow rng = load_rng(a.states, a.n_threads, tid);
    for (uint32_t sample = 0; sample < a.samples_per_thread; ++sample) {
      double real, imag;
      if (from_cells) {
        next_sample<true>(fa, rng, real, imag);
      } else {
        next_sample<false>(fa, rng, real, imag);
      }
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
      if (!to_mask) st.recorded++;
      r = real;
      i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = a.burning_ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i);
        st.replay_steps++;
        int row, col;
        if (pixel_of(r, i, cv, row, col)) {
          if (to_mask) {  // the first in-canvas point: the sample's cell reaches the canvas
            mark_cell(fa, real, imag);
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
// Every lane owns one reference thread (its generator, its samples_per_thread samples) and works on one sample at a
// time.  The wave advances in ROUNDS of kFocusRound steps; in a round each lane makes up to kFocusRound steps of its own
// phase, and between rounds each lane, on its own, does its bookkeeping:
//   ITERATE  z_k -> z_{k+kFocusRound} (fewer at max_iter), testing |z|^2 > 4 after every step.  A lane that escapes at
//            its n-th step (the reference's k = n - 1) notes n and idles to the round's end (ESCAPED); there the accept
//            filter sends it to NEXT (too fast) or REPLAY.  At k a multiple of kChunk: z_k == the saved point bit for
//            bit -> the orbit is an exact cycle of points that all passed the test, so it never escapes: counted as the
//            reference counts it (never_escaped, max_iter iterate steps), the steps not made in skipped_steps; else
//            Brent's save.  At k == max_iter: never escaped.
//   REPLAY   z_1 .. z_n from z_0 = c, the same steps bit for bit, so the n-th is the one that escapes: each binned; the
//            histogram sink adds every in-canvas point, the mask sink stops at the first.
//   NEXT     draw the lane's next sample (rejecting cardioid and bulb), or finish.
// Rounds divide kChunk, so an iterating lane is at a chunk boundary exactly when k % kChunk == 0.
constexpr int kFocusRound = 12;
static_assert(kChunk % kFocusRound == 0, "an iterating lane meets every chunk boundary at a round's end");

enum : int { kFocusNext = 0, kFocusIterate = 1, kFocusReplay = 2, kFocusEscaped = 3, kFocusDone = 4 };

template <bool kCells, bool kMask, bool kShip>
__global__ void __launch_bounds__(256) draw_focus_kernel(FocusArgs fa) {
  const DrawArgs &a = fa.d;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  const Canvas cv = make_canvas(a);
  const int max_iter = a.max_iter;
  LaneStats st;
  Xorwow rng = {0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) rng = load_rng(a.states, a.n_threads, tid);
  uint32_t left = valid ? a.samples_per_thread : 0u;
  int phase = kFocusNext;
  double cr = 0.0, ci = 0.0, r = 0.0, i = 0.0;  // the sample and its orbit: z_k
  double sr = 0.0, si = 0.0;                      // ITERATE: the saved point
  int k = 0;                                      // index of z
  int saved = 0;                                  // ITERATE: index of the saved point (0: none yet)
  int end = 0;                                    // ESCAPED, REPLAY: the step that escapes
  while (true) {
    // ---- between rounds: each lane's bookkeeping --------------------------------------------------------------
    if (phase == kFocusNext) {
      while (left > 0u) {
        left--;
        next_sample<kCells>(fa, rng, cr, ci);
        st.samples++;
        if (!kShip && (in_main_cardioid(cr, ci) || in_order2_bulb(cr, ci))) {
          st.rejected++;
          continue;
        }
        if (max_iter <= 0) {  // IterateMandelbrot returns max at once
          st.never_escaped++;
          continue;
        }
        r = cr;
        i = ci;
        k = 0;
        saved = 0;
        phase = kFocusIterate;
        break;
      }
      if (phase == kFocusNext) phase = kFocusDone;
    }
    if (__ballot(phase != kFocusDone) == 0ull) break;
    // ---- one round ----------------------------------------------------------------------------------------------
    const int limit = phase == kFocusIterate ? max_iter : end;
    const int stop = phase == kFocusDone ? k : (limit - k < kFocusRound ? limit : k + kFocusRound);
#pragma unroll 2
    for (int t = 0; t < kFocusRound; ++t) {
      if (k < stop) {
        const double m = focus_step<kShip>(cr, ci, r, i);
        ++k;
        if (phase == kFocusReplay) {
          int row, col;
          if (pixel_of(r, i, cv, row, col)) {
            if (kMask) {  // the first in-canvas point ends the replay
              mark_cell(fa, cr, ci);
              st.recorded++;
              st.replay_steps += (unsigned long long) k;
              phase = kFocusNext;
              k = stop;
            } else {
              add_to_pixel(a.hist, cv, row, col, 1ull);
              st.increments++;
            }
          }
        } else if (m > 4.0) {  // escaped at z_k
          end = k;
          phase = kFocusEscaped;
          k = stop;  // no more steps this round
        }
      }
    }
    if (phase == kFocusReplay) {
      if (k == end) {
        if (kMask) st.replay_steps += (unsigned long long) end;  // no point on the canvas
        phase = kFocusNext;
      }
    } else if (phase == kFocusEscaped) {
      st.iterate_steps += (unsigned long long) end;
      if (end - 1 < a.min_iter) {
        st.too_fast++;
        phase = kFocusNext;
      } else {
        if (!kMask) {
          st.recorded++;
          st.replay_steps += (unsigned long long) end;
        }
        r = cr;
        i = ci;
        k = 0;
        phase = kFocusReplay;
      }
    } else if (phase == kFocusIterate) {
      const bool boundary = (k % kChunk) == 0;
      if (k == max_iter) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) max_iter;
        phase = kFocusNext;
      } else if (boundary && saved > 0 && same_bits(r, i, sr, si)) {
        st.never_escaped++;
        st.iterate_steps += (unsigned long long) max_iter;
        st.reserved += (unsigned long long) (max_iter - k);
        phase = kFocusNext;
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
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  const uint32_t blocks = (a.d.n_threads + 255u) / 256u;
  const bool from_cells = a.cells != nullptr, to_mask = a.mask != nullptr;
  if (lockstep) {
    hipLaunchKernelGGL(draw_focus_simple_kernel, dim3(blocks), dim3(256), 0, stream, a);
  } else if (from_cells && !to_mask) {  // the focused draw
    launch_product<true, false>(a, blocks, stream);
  } else if (!from_cells && to_mask) {  // the probe
    launch_product<false, true>(a, blocks, stream);
  } else if (!from_cells && !to_mask) {  // a normal render through this kernel (the tests' check against the oracle)
    launch_product<false, false>(a, blocks, stream);
  } else {
    return hipErrorInvalidValue;  // (cells, mask): a probe of a focused stream is not defined
  }
  return hipGetLastError();
}

}  // namespace cb
