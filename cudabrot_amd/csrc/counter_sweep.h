// counter_sweep.h -- what the device files of the output stage share (tonemap.hip, exposure.hip, equalize.hip, color.hip;
// density.hip for the host helpers): the streaming sweep of the u64 counters, the wave-aggregated count into block-private
// bins, the two-pixels-per-lane lookup loop with its big-endian store, and the host's launch arithmetic and clean-up.  One
// definition of each: a fix to the sweep's head or tail is made here, once.
#pragma once

#include "color_math.h"
#include "kernels.h"

namespace cb {

constexpr uint32_t kSweepThreads = 256;  // lanes of every kernel of the output stage but the colour stage's own
constexpr uint32_t kSweepBlocks = 1024;  // the sweep's grid cap: four blocks per CU
constexpr uint32_t kVector = 2;          // counters per 16-byte load
constexpr uint32_t kLoads = 4;           // loads a lane has in flight
constexpr unsigned long long kBlockSweep = (unsigned long long) kSweepThreads * kLoads * kVector;  // counters per turn
constexpr unsigned long long kMaxCounters = 1ull << 40;
// A u32 bin cannot overflow: a block counts at most the counters it reads, ceil(n / sweep) of its kBlockSweep-counter
// turns, and n <= kMaxCounters is enforced by the callers.
static_assert(kMaxCounters / kSweepBlocks + kBlockSweep < (1ull << 31), "a block's u32 bins hold what it reads");

// Every counter of hist[0, n) once, to f -- zero for the slots past the end.  f is called by every lane of the block the
// same number of times (the loop bounds are the block's), so it may ballot.  hist is 8-byte aligned; where it is not
// 16-byte aligned its first counter is taken apart, and so is a last one without a partner: the 16-byte loads are aligned
// and stay inside the buffer.  The two ends go to lanes 0 and 1 of block 0.
template <class F>
__device__ __forceinline__ void for_each_counter(const unsigned long long *hist, unsigned long long n, F f) {
  const unsigned long long head = (reinterpret_cast<uintptr_t>(hist) & 8u) ? 1ull : 0ull;  // n >= 1
  const ulonglong2 *vec = reinterpret_cast<const ulonglong2 *>(hist + head);
  const unsigned long long pairs = (n - head) / kVector;
  constexpr unsigned long long kTurn = (unsigned long long) kSweepThreads * kLoads;  // pairs a block takes per turn
  for (unsigned long long base = (unsigned long long) blockIdx.x * kTurn; base < pairs;
       base += (unsigned long long) gridDim.x * kTurn) {
    ulonglong2 q[kLoads];
#pragma unroll
    for (uint32_t j = 0; j < kLoads; ++j) {
      const unsigned long long at = base + (unsigned long long) j * kSweepThreads + threadIdx.x;
      q[j] = make_ulonglong2(0ull, 0ull);
      if (at < pairs) q[j] = vec[at];
    }
#pragma unroll
    for (uint32_t j = 0; j < kLoads; ++j) {
      f(q[j].x);
      f(q[j].y);
    }
  }
  if (blockIdx.x == 0) {
    const unsigned long long last = head + pairs * kVector;  // < n: one counter without a partner
    unsigned long long c = 0;
    if (threadIdx.x == 0 && head) c = hist[0];
    if (threadIdx.x == 1 && last < n) c = hist[last];
    f(c);
  }
}

// Lanes with `active` add 1 to lds[bin]: the lanes that share the first active lane's bin add once, by popcount, the
// rest are LDS atomics.  Every lane of the wave takes part (the callers keep it converged).
__device__ __forceinline__ void wave_count(uint32_t *lds, uint32_t bin, bool active) {
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;
  const int first = __ffsll((long long) act) - 1;
  const uint32_t lead = (uint32_t) __builtin_amdgcn_readlane((int) bin, first);
  const bool same = active && bin == lead;
  const unsigned long long mate = __ballot(same);
  if (same) {
    if ((int) (threadIdx.x & 63u) == first) atomicAdd(&lds[lead], (uint32_t) __popcll(mate));
  } else if (active) {
    atomicAdd(&lds[bin], 1u);
  }
}

// out_be[i] = value(hist[i]) as big-endian u16, two pixels per lane: one 4-byte store, and a 2-byte one for a last pixel
// without a partner.  The grid is pairs_grid's.
template <class F>
__device__ __forceinline__ void map_pairs(const unsigned long long *hist, unsigned long long n, uint16_t *out_be, F value) {
  const unsigned long long stride = (unsigned long long) gridDim.x * kSweepThreads * 2ull;
  for (unsigned long long i = ((unsigned long long) blockIdx.x * kSweepThreads + threadIdx.x) * 2ull; i < n; i += stride) {
    const uint32_t a = color_swap16(value(hist[i]));
    if (i + 1 < n) {
      const uint32_t b = color_swap16(value(hist[i + 1]));
      *reinterpret_cast<uint32_t *>(out_be + i) = a | (b << 16);  // n even or not: i is even
    } else {
      out_be[i] = (uint16_t) a;
    }
  }
}

// ---- the host's side ----

inline uint32_t sweep_grid(unsigned long long n) {  // of a for_each_counter kernel
  const unsigned long long blocks = (n + kBlockSweep - 1) / kBlockSweep;
  return (uint32_t) (blocks == 0 ? 1 : (blocks > kSweepBlocks ? kSweepBlocks : blocks));
}

inline uint32_t pairs_grid(unsigned long long n) {  // of a map_pairs kernel, and of hist_max_kernel
  unsigned long long blocks = (n / 2 + kSweepThreads) / kSweepThreads;
  if (blocks > 256ull * 16ull) blocks = 256ull * 16ull;
  return (uint32_t) (blocks ? blocks : 1);
}

inline bool tone_mode_ok(int mode) { return mode == CB_TONE_AUTO || mode == CB_TONE_LUT || mode == CB_TONE_THRESHOLDS; }

#define CB_HIP_TRY(expr)                    \
  do {                                      \
    const hipError_t e_ = (expr);           \
    if (e_ != hipSuccess) return (int) e_;  \
  } while (0)

struct DeviceBuffer {  // freed on every return path
  void *p = nullptr;
  ~DeviceBuffer() {
    if (p) (void) hipFree(p);
  }
};

}  // namespace cb
