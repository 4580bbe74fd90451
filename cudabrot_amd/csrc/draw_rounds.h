// draw_rounds.h -- what the kernels with one reference thread per lane share (kernels.hip's draw_simple_kernel,
// draw_anti.hip, draw_focus.hip, draw_plot.hip): the per-lane counters, the uniform
// sample, the reference's escape-index loop for the lock-step kernels, and the round scheduler of the product kernels
// with the escape accounting of its modes.
#pragma once

#include "draw_common.h"

namespace cb {

// Per-lane statistics, summed over the wave at kernel end (one atomic per counter per wave); `reserved` is
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

// The sample of the normal stream: c uniform over [-2, 2)^2, two draws per coordinate.
__device__ __forceinline__ void uniform_sample(Xorwow &rng, double &real, double &imag) {
  real = sample_coordinate(rng);
  imag = sample_coordinate(rng);
}

// IterateMandelbrot (cudabrot.cu:319-340) for the lock-step kernels: the k of the first z_{k+1} with |z|^2 > 4, or
// max_iter when none of z_1 .. z_max_iter escapes (at once for max_iter <= 0).
__device__ __forceinline__ int escape_index(double real, double imag, int max_iter, bool ship) {
  double r = real, i = imag;
  for (int it = 0; it < max_iter; ++it) {
    if ((ship ? mandel_step_ship(real, imag, r, i) : mandel_step(real, imag, r, i)) > 4.0) return it;
  }
  return max_iter;
}

template <bool kShip>
__device__ __forceinline__ double orbit_step(double cr, double ci, double &r, double &i) {
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

// ------------------------------------------------------------------------------------------------
// The round scheduler: lanes refilled from their own subsequence, exact-periodicity check at chunk boundaries
// ------------------------------------------------------------------------------------------------
//
// Every lane owns one reference thread (its generator, its samples_per_thread samples) and works on one sample at a
// time.  The wave advances in ROUNDS of kRound steps; in a round each lane makes up to kRound steps of its own phase,
// and between rounds each lane, on its own, does its bookkeeping.  What a kernel adds is its MODE: a struct with the
// step (kShip, or a step of its own: round_step below), whatever per-lane state it needs beyond RoundLane, and four
// inlined hooks, named where they are called (more, optional: round_converged, the state hooks and round_again below):
//   NEXT     the lane's next sample, or DONE when it has none left.  mode.next draws c and says what becomes of it: it
//            is iterated, or retired as drawn -- rejected (cardioid, bulb), or proven interior and counted as the
//            reference counts a sample that never escapes -- and the next one drawn.  (max_iter 0 needs no case of its
//            own: ITERATE makes no step and is at k == max_iter at once.)
//   ITERATE  z_k -> z_{k+kRound} (fewer at max_iter), testing |z|^2 > 4 after every step.  A lane that escapes at its
//            n-th step (the reference's k = n - 1) notes n in `end` and idles to the round's end (ESCAPED); there
//            mode.escaped counts the sample and decides: true, REPLAY z_1 .. z_n.
//            At k a multiple of kChunk: z_k == the saved point z_saved bit for bit -> the orbit is the exact cycle
//            z_saved .. z_{k-1} repeated, every point of which passed the test, so it never escapes;
//            else Brent's save.  On such a cycle, or at k == max_iter, mode.never_escapes counts the sample (the steps
//            not made go to skipped_steps) and decides: true, REPLAY up to the `end` it has set.
//   REPLAY   z_1 .. z_end from z_0 = c, the same steps bit for bit; mode.point bins each, and may end the replay there
//            by returning true.  Where the mode has the chaining hook (round_again), another such pass may follow.
// A lane that completes a phase mid-round idles to the round's end: kRound steps are the grain of the refill.  Rounds
// divide kChunk, so an iterating lane is at a chunk boundary exactly when k % kChunk == 0.
constexpr int kRound = 12;
static_assert(kChunk % kRound == 0, "an iterating lane meets every chunk boundary at a round's end");

enum : int { kSampleIterate = 0, kSampleRejected = 1, kSampleInterior = 2 };  // what mode.next returns
enum : int { kRoundNext = 0, kRoundIterate = 1, kRoundReplay = 2, kRoundEscaped = 3, kRoundDone = 4 };

struct RoundLane {
  int max_iter;                                   // wave-uniform: the launch's, negative taken as 0
  double cr = 0.0, ci = 0.0, r = 0.0, i = 0.0;    // the sample and its orbit: z_k
  double sr = 0.0, si = 0.0;                      // ITERATE: the saved point z_saved
  int k = 0;                                      // index of z
  int saved = 0;                                  // ITERATE: index of the saved point (0: none yet)
  int end = 0;                                    // ESCAPED: the step that escaped; REPLAY: the last index replayed
};

// The step of a round: the mode's own `double step(RoundLane &)` where it has one (it advances l.r, l.i and returns
// |z|^2), else the reference's step, picked by Mode::kShip.  ITERATE and REPLAY make the same call.
template <class Mode>
__device__ __forceinline__ auto round_step(Mode &mode, RoundLane &l, int) -> decltype(mode.step(l)) {
  return mode.step(l);
}
template <class Mode>
__device__ __forceinline__ double round_step(Mode &, RoundLane &l, long) {
  return orbit_step<Mode::kShip>(l.cr, l.ci, l.r, l.i);
}

// The convergent hook of a round: the mode's own `void converged(RoundLane &, LaneStats &, bool last)` where it has one,
// else nothing.  run_rounds calls it with all 64 lanes of the wave active -- after every step of a round, whatever each
// lane did in it, and once more (last = true) when no lane has work left, before the generators and the counters are
// stored -- so a mode may do there what needs the whole wave: cross-lane work on what its lanes noted in mode.point.
template <class Mode>
__device__ __forceinline__ auto round_converged(Mode &mode, RoundLane &l, LaneStats &st, bool last, int)
    -> decltype(mode.converged(l, st, last)) {
  return mode.converged(l, st, last);
}
template <class Mode>
__device__ __forceinline__ void round_converged(Mode &, RoundLane &, LaneStats &, bool, long) {}

// The state hooks of a round, for a step with memory -- one whose next point is a function of more than (z, c), so that
// the mode keeps the rest of the orbit's state per lane.  Each is the mode's own where it has one, else nothing:
//   void start(RoundLane &)   the orbit begins: run_rounds has set z = z_0 and k = 0, for ITERATE or for REPLAY, and the
//                             mode sets the rest of its state to its beginning, so that the replay retraces the iteration;
//   void save(RoundLane &)    run_rounds has saved z as the point of the exact-periodicity test, and the mode saves the rest;
//   bool same(RoundLane &)    the rest of the state equals what save kept, bit for bit.  round_same forms the conjunction
//                             with the scheduler's own same_bits(z, z_saved): a mode can only make the test stricter.  It
//                             has to, where its step has memory: z_k == z_saved alone says nothing about z_{k+1} then.
template <class Mode>
__device__ __forceinline__ auto round_start(Mode &mode, RoundLane &l, int) -> decltype(mode.start(l)) {
  return mode.start(l);
}
template <class Mode>
__device__ __forceinline__ void round_start(Mode &, RoundLane &, long) {}
template <class Mode>
__device__ __forceinline__ auto round_save(Mode &mode, RoundLane &l, int) -> decltype(mode.save(l)) {
  return mode.save(l);
}
template <class Mode>
__device__ __forceinline__ void round_save(Mode &, RoundLane &, long) {}
template <class Mode>
__device__ __forceinline__ auto round_same(Mode &mode, RoundLane &l, bool z_same, int) -> decltype(mode.same(l)) {
  return z_same && mode.same(l);
}
template <class Mode>
__device__ __forceinline__ bool round_same(Mode &, RoundLane &, bool z_same, long) {
  return z_same;
}

// The chaining hook of a round: the mode's own `bool again(RoundLane &, LaneStats &)` where it has one, else false.
// run_rounds calls it between rounds when a lane's REPLAY-like pass has ended -- at l.k == l.end, or because mode.point
// returned true -- and on true starts another pass as it started the first: z = z_0, k = 0, round_start, up to the `end`
// the mode has set.  A mode that walks from somewhere else than z_0 places z there in its `start` (draw_periods.hip: the
// period search runs as such a pass, scheduled like any other, and the replay of the orbit is chained after it).
template <class Mode>
__device__ __forceinline__ auto round_again(Mode &mode, RoundLane &l, LaneStats &st, int) -> decltype(mode.again(l, st)) {
  return mode.again(l, st);
}
template <class Mode>
__device__ __forceinline__ bool round_again(Mode &, RoundLane &, LaneStats &, long) {
  return false;
}

// The escape accounting of an escape render's mode (not the anti-Buddhabrot's, which records the other samples).
// mode.escaped: the sample went l.end steps; through the accept filter min <= k < max, k = l.end - 1, to REPLAY (true).
// recorded = false: the mode counts `recorded` itself (the mask sink, at the point that ends its replay).
__device__ __forceinline__ bool count_escaped(const RoundLane &l, int min_iter, LaneStats &st, bool recorded = true) {
  st.iterate_steps += (unsigned long long) l.end;
  if (l.end - 1 < min_iter) {
    st.too_fast++;
    return false;
  }
  if (recorded) st.recorded++;
  st.replay_steps += (unsigned long long) l.end;
  return true;
}
// mode.never_escapes: counted as the reference counts it, the steps not made in skipped_steps; nothing to replay.
__device__ __forceinline__ bool count_never_escapes(const RoundLane &l, LaneStats &st) {
  st.never_escaped++;
  st.iterate_steps += (unsigned long long) l.max_iter;
  st.reserved += (unsigned long long) (l.max_iter - l.k);  // 0 at k == max_iter
  return false;
}

template <class Mode>
__device__ __forceinline__ void run_rounds(const DrawArgs &a, Mode &mode) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = tid < a.n_threads;
  LaneStats st;
  Xorwow rng = {0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) rng = load_rng(a.states, a.n_threads, tid);
  uint32_t left = valid ? a.samples_per_thread : 0u;
  int phase = kRoundNext;
  RoundLane l;
  l.max_iter = a.max_iter > 0 ? a.max_iter : 0;
  while (true) {
    // ---- between rounds: each lane's bookkeeping --------------------------------------------------------------
    if (phase == kRoundNext) {
      while (left > 0u) {
        left--;
        st.samples++;
        const int drawn = mode.next(rng, l);
        if (drawn == kSampleRejected) {
          st.rejected++;
          continue;
        }
        if (drawn == kSampleInterior) {  // as the reference counts it, every step of it skipped
          st.never_escaped++;
          st.iterate_steps += (unsigned long long) l.max_iter;
          st.reserved += (unsigned long long) l.max_iter;
          continue;
        }
        l.r = l.cr;
        l.i = l.ci;
        l.k = 0;
        l.saved = 0;
        round_start(mode, l, 0);
        phase = kRoundIterate;
        break;
      }
      if (phase == kRoundNext) phase = kRoundDone;
    }
    if (__ballot(phase != kRoundDone) == 0ull) break;
    // ---- one round ----------------------------------------------------------------------------------------------
    const int limit = phase == kRoundIterate ? l.max_iter : l.end;
    const int stop = phase == kRoundDone ? l.k : (limit - l.k < kRound ? limit : l.k + kRound);
#pragma unroll 2
    for (int t = 0; t < kRound; ++t) {
      if (l.k < stop) {
        const double m = round_step(mode, l, 0);
        ++l.k;
        if (phase == kRoundReplay) {
          if (mode.point(l, st)) {
            phase = kRoundNext;
            l.k = stop;
          }
        } else if (m > 4.0) {  // escaped at z_k
          l.end = l.k;
          phase = kRoundEscaped;
          l.k = stop;  // no more steps this round
        }
      }
      round_converged(mode, l, st, false, 0);
    }
    bool replay = false;
    if (phase == kRoundNext) {  // mode.point ended the REPLAY
      replay = round_again(mode, l, st, 0);
    } else if (phase == kRoundReplay) {
      if (l.k == l.end) {
        phase = kRoundNext;
        replay = round_again(mode, l, st, 0);
      }
    } else if (phase == kRoundEscaped) {
      replay = mode.escaped(l, st);
      if (!replay) phase = kRoundNext;
    } else if (phase == kRoundIterate) {
      const bool boundary = (l.k % kChunk) == 0;
      const bool cycle = round_same(mode, l, boundary && l.saved > 0 && same_bits(l.r, l.i, l.sr, l.si), 0);
      if (cycle || l.k == l.max_iter) {
        replay = mode.never_escapes(l, st, cycle);
        if (!replay) phase = kRoundNext;
      } else if (boundary && brent_save((uint32_t) (l.k / kChunk))) {
        l.sr = l.r;
        l.si = l.i;
        l.saved = l.k;
        round_save(mode, l, 0);
      }
    }
    if (replay) {
      l.r = l.cr;
      l.i = l.ci;
      l.k = 0;
      round_start(mode, l, 0);
      phase = kRoundReplay;
    }
  }
  round_converged(mode, l, st, true, 0);
  if (valid) store_rng(a.states, a.n_threads, tid, rng);
  flush_stats(a.counters, st);
}

}  // namespace cb
