// draw_frames.hip -- the frames render (include/cudabrot_amd.h, "Frames render"): a projected render or a
// Julia render (draw_plot.hip) whose visited points are plotted with F matrices P_f instead of one, frame f into plane f of
// the histogram (planes plane_pixels counters apart):
//   K_u = fma(P_f[0][2], c_re, P_f[0][3] * c_im)
//   u   = fma(P_f[0][0], z_re, fma(P_f[0][1], z_im, K_u))      v likewise from row 1
// -- the projected render's four fused operations and its binning, F times per point.  Sample stream, rejection, interior
// map, iteration, escape index, accept filter and replayed points are the projected render's (a sampled c) or the Julia
// render's (a fixed one), unchanged, and so is every counter but increments, which counts the points added over all planes.
//
// Kernels (the number: cb_debug_last_draw_kernel)
//   draw_frames_simple_kernel        the definition verbatim, one lane per reference thread in lock-step, no early-out, a
//                                    loop over the frames at every point; step, degree, formula and Julia-or-not are
//                                    run-time arguments.  No LDS.  Validation baseline (23).
//   draw_frames_kernel<Step, kJulia> the product kernel (22): the round scheduler of draw_rounds.h with FramesMode, which
//                                    wraps PlotMode / JuliaMode of draw_plot.h as DepthMode does: step, NEXT (with the
//                                    interior map under PlotMode's own rule), ESCAPED's accounting and the never-escaping
//                                    case are theirs.  The plot is not made where the point is visited: see below.  One
//                                    instance per step (13) and per source of c (2): 26.
//
// The point queue.  mode.point runs under the scheduler's divergent REPLAY branch: a loop over F frames there would run
// with the replaying lanes alone while the iterating lanes of the wave wait F times longer per step, and from F = 8 on the
// per-frame work (about 12 fp64 operations, a binning and an atomic) is the kernel's work.  So the point is only NOTED
// there, and at the scheduler's convergent hook -- all 64 lanes active, after every step of a round -- the lanes that
// noted one append it to a queue in LDS that belongs to their wave alone: slot = queue count + rank among the appending
// lanes (a ballot and mbcnt), the count wave-uniform.  A queue that then holds 64 records or more is DRAINED 64 lanes
// wide: lane j takes one of the 64 newest records and loops over the frames, the matrix of each read with wave-uniform
// (scalar) loads, and makes the add into plane f.  Sums do not depend on their order, so neither the histogram nor the
// counters depend on which lane drains what.  After the last round the remainder (fewer than 64) is drained by the lanes
// below the count.
//   Capacity: at most 64 records are appended between two hooks and a drain leaves at most 63, so 128 slots never
//   overflow.  The record is (z_re, z_im, c_re, c_im) -- 4 KiB per wave, 16 KiB per block -- or (z_re, z_im) alone under a
//   fixed c, whose K_u and K_v are wave-uniform per frame: 2 KiB per wave, 8 KiB per block.  One array per component, so
//   that 64 consecutive slots are 64 consecutive doubles.
//   No __syncthreads: the lanes of the other waves are in other rounds.  Wavefront-scope fences keep the compiler from
//   moving the LDS accesses across append and drain; the hardware executes a wave's LDS instructions in order.
// No workspace, no carry: every launch is complete, and lane t advances generator t by exactly its samples.
#include "draw_depth.h"

namespace cb {

namespace {

// The matrices as the kernels read them: the constant address space, so that a wave-uniform index is a scalar load
// whatever the atomics around it write (the matrices are written before the launch and by nobody after).
typedef const double __attribute__((address_space(4))) *FrameMatrices;
__device__ __forceinline__ FrameMatrices frame_matrices(const double *frames) {
  return (FrameMatrices) (unsigned long long) frames;
}

// The kernel's arguments read afresh, as draw_depth.h's fresh_depth_args reads a DepthArgs: what the plot of an accepted
// orbit alone needs (the matrices, their number, the distance of the planes) is loaded where it is used in the lock-step
// kernel and holds no scalar register across the iterate loop, where it would otherwise spill.
typedef const FramesArgs __attribute__((address_space(4))) *FramesKernelArgs;
__device__ __forceinline__ FramesKernelArgs fresh_frames_args() {
  FramesKernelArgs p = (FramesKernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// One matrix, loaded: eight wave-uniform doubles.
struct FrameMatrix {
  double p[8];
};
__device__ __forceinline__ FrameMatrix load_matrix(FrameMatrices frames, int f) {
  FrameMatrix m;
#pragma unroll
  for (int j = 0; j < 8; ++j) m.p[j] = frames[8 * f + j];
  return m;
}

// The plot of one point with every matrix: returns the points added.  The matrix of the next frame is asked for before
// this frame's is used (the last frame asks for itself again), so that a scalar load's latency lies under a frame's
// arithmetic; kAhead false: one matrix at a time, for the kernel whose scalar registers that second matrix would spill.
template <bool kAhead>
__device__ __forceinline__ unsigned long long plot_frames(FrameMatrices frames, int n_frames, unsigned long long *hist,
                                                          unsigned long long plane_pixels, const Canvas &cv, double r,
                                                          double i, double c_re, double c_im) {
  unsigned long long added = 0ull;
  FrameMatrix m = load_matrix(frames, 0);
#pragma unroll 1
  for (int f = 0; f < n_frames; ++f) {
    FrameMatrix next;
    if constexpr (kAhead) {
      next = load_matrix(frames, f + 1 < n_frames ? f + 1 : f);
    } else if (f > 0) {
      m = load_matrix(frames, f);
    }
    const double ku = project_constant(m.p[2], m.p[3], c_re, c_im);
    const double kv = project_constant(m.p[6], m.p[7], c_re, c_im);
    const double u = project_point(m.p[0], m.p[1], r, i, ku);
    const double v = project_point(m.p[4], m.p[5], r, i, kv);
    int row, col;
    if (pixel_of(u, v, cv, row, col)) {
      add_to_pixel(hist + (unsigned long long) f * plane_pixels, cv, row, col, 1ull);
      added++;
    }
    if constexpr (kAhead) m = next;
  }
  return added;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The lock-step kernel: the definition, verbatim
// ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) draw_frames_simple_kernel(FramesArgs fa) {
  const PlotArgs &pa = fa.p;
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
      const FramesKernelArgs now = fresh_frames_args();
      const FrameMatrices frames = frame_matrices(now->frames);
      double r = real, i = imag;
      for (int it = 0; it <= a.max_iter; ++it) {  // bounded so that a wave always terminates
        const double m = depth_step(f, deg, ship, c_re, c_im, r, i);
        st.replay_steps++;
        st.increments += plot_frames<false>(frames, now->n_frames, a.hist, now->plane_pixels, cv, r, i, c_re, c_im);
        if (m > 4.0) break;
        if (it == a.max_iter) st.status |= CB_STATUS_REPLAY_RUNAWAY;
      }
    }
    store_rng(a.states, a.n_threads, tid, rng);
  }
  flush_stats(a.counters, st);
}

// ------------------------------------------------------------------------------------------------
// draw_frames_kernel: lanes refilled from their own subsequence, the plot queued and made 64 lanes wide
// ------------------------------------------------------------------------------------------------

namespace {

constexpr int kQueueSlots = 128;  // per wave: 64 appended between two hooks on top of the 63 a drain leaves, at the most
constexpr int kBlockWaves = 256 / 64;

// The queue of one block: a wave's records, one array per component.
template <bool kJulia>
struct PointQueues {
  static constexpr int kComponents = kJulia ? 2 : 4;  // (z_re, z_im[, c_re, c_im])
  double at[kBlockWaves][kComponents][kQueueSlots];
};

// The round scheduler of draw_rounds.h with FramesMode: PlotMode (a sampled c) or JuliaMode (a fixed one) of draw_plot.h
// with another plot.  `point` notes that the lane has visited z = (l.r, l.i), which the lane still holds at the hook that
// follows the step; `converged` appends the noted points to the wave's queue and drains it (the commentary at the top).
// (The base's ESCAPED also makes the two constants of a sampled c for pa.p, which nothing reads: the compiler drops them.)
template <class Step, bool kJulia>
struct FramesMode {
  typename std::conditional<kJulia, JuliaMode<Step>, PlotMode<Step>>::type base;
  const FramesArgs &fa;
  double (*const queue)[kQueueSlots];  // the wave's arrays: [component][slot]
  int count = 0;                       // records in the queue: wave-uniform
  bool noted = false;                  // the lane visited a point in the step before this hook

  __device__ __forceinline__ double step(RoundLane &l) { return base.step(l); }
  __device__ __forceinline__ int next(Xorwow &rng, RoundLane &l) { return base.next(rng, l); }
  __device__ __forceinline__ bool escaped(RoundLane &l, LaneStats &st) { return base.escaped(l, st); }
  __device__ __forceinline__ bool never_escapes(RoundLane &l, LaneStats &st, bool cycle) {
    return base.never_escapes(l, st, cycle);
  }

  __device__ __forceinline__ bool point(RoundLane &, LaneStats &) {
    noted = true;
    return false;
  }

  // Records [first, first + n) of the queue, n <= 64: lane j < n plots record first + j with every matrix.
  __device__ __forceinline__ void drain(int first, int n, LaneStats &st) {
    const int lane = lane_id();
    if (lane < n) {
      const int slot = first + lane;  // < kQueueSlots: first + n <= count
      const double r = queue[0][slot], i = queue[1][slot];
      double c_re, c_im;
      if constexpr (kJulia) {
        c_re = base.c_re;
        c_im = base.c_im;
      } else {
        c_re = queue[2][slot];
        c_im = queue[3][slot];
      }
      const Plot &plot = base.plot;
      st.increments += plot_frames<true>(frame_matrices(fa.frames), fa.n_frames, plot.pa.d.hist, fa.plane_pixels, plot.cv, r, i,
                                   c_re, c_im);
    }
  }

  __device__ __forceinline__ void converged(RoundLane &l, LaneStats &st, bool last) {
    if (!last) {
      const unsigned long long appending = __ballot(noted);
      if (appending != 0ull) {
        if (noted) {
          const int slot = count + mask_prefix(appending);  // <= 63 + 63
          queue[0][slot] = l.r;
          queue[1][slot] = l.i;
          if constexpr (!kJulia) {
            queue[2][slot] = l.cr;
            queue[3][slot] = l.ci;
          }
          noted = false;
        }
        count += __popcll(appending);
      }
      if (count < 64) return;
    } else if (count == 0) {
      return;
    }
    // what the appending lanes wrote is what the draining lanes read: the same wave, in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = count < 64 ? count : 64;
    drain(count - n, n, st);
    count -= n;
    // the slots just read are written again only behind this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

}  // namespace

// The body stands in the kernel, not in a function the kernel calls.
template <class Step, bool kJulia>
__global__ void __launch_bounds__(256) draw_frames_kernel(FramesArgs fa) {
  __shared__ PointQueues<kJulia> queues;
  const PlotArgs &pa = fa.p;
  double(*const queue)[kQueueSlots] = queues.at[threadIdx.x >> 6];
  if constexpr (kJulia) {
    FramesMode<Step, true> mode{{{pa, make_canvas(pa.d)}, pa.c[0], pa.c[1]}, fa, queue};
    run_rounds(pa.d, mode);
  } else {
    FramesMode<Step, false> mode{{{pa, make_canvas(pa.d)}}, fa, queue};
    run_rounds(pa.d, mode);
  }
}

namespace {

typedef void (*FramesKernel)(FramesArgs);

// The product kernels of one step, [fixed c], and every one there is, by step (draw_plot.h, plot_step_index).
struct StepKernels {
  FramesKernel by[2];
};
#define CB_ROW(Step) {{draw_frames_kernel<Step, false>, draw_frames_kernel<Step, true>}},
constexpr StepKernels kFramesKernels[] = {CB_PLOT_STEPS(CB_ROW)};
#undef CB_ROW
static_assert(sizeof(kFramesKernels) / sizeof(kFramesKernels[0]) == kPlotSteps, "one row per step");

}  // namespace

hipError_t launch_draw_frames(const FramesArgs &fa, bool lockstep, hipStream_t stream) {
  const PlotArgs &a = fa.p;
  if (!plot_launch_ok(a)) return hipErrorInvalidValue;
  if (a.palette != 0 || a.lut != nullptr) return hipErrorInvalidValue;  // no table: 3 F planes are out of scope
  // every plane a frame adds to is a plane of the histogram, and the planes are one w x F*h image to the tone map
  if (fa.frames == nullptr || fa.n_frames < 1 || fa.n_frames > CB_FRAMES_MAX || a.d.w <= 0 || a.d.h <= 0 ||
      fa.plane_pixels != (unsigned long long) a.d.w * (unsigned long long) a.d.h ||
      (long long) fa.n_frames * (long long) a.d.h > 0x7fffffffLL) {
    return hipErrorInvalidValue;
  }
  if (a.d.n_threads == 0 || a.d.samples_per_thread == 0) return hipSuccess;
  FramesKernel kernel = nullptr;
  if (lockstep) {
    kernel = draw_frames_simple_kernel;
  } else {
    kernel = kFramesKernels[plot_step_index(a)].by[a.julia != 0];
  }
  hipLaunchKernelGGL(kernel, dim3((a.d.n_threads + 255u) / 256u), dim3(256), 0, stream, fa);
  return hipGetLastError();
}

}  // namespace cb
