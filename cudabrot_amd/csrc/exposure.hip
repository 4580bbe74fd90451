// exposure.hip -- the white clip on the device (include/cudabrot_amd.h, "White clip"): the white point of
// an image as an exact order statistic of its u64 counters, and the tone map against it.
//
// white = the (r + 1)-th largest counter among the lit ones (count > 0), r made by the host (cb_white_rank: the only
// fp64 of the definition).  A radix select, most significant byte first:
//   pass 0        one sweep: the largest counter and the number of lit ones;
//   digit passes  one per significant byte of the maximum: a 256-bin count of that byte over the lit counters whose
//                 higher bytes equal the prefix chosen so far; 2 KB come back and the host walks the bins from the top
//                 (color_select_high, the walk of the colour stage) to the bin that holds the rank.
// At most nine streaming reads of the histogram, once per image; r = 0 (no clip) ends after pass 0.  What lies above the
// chosen bin in each pass is above white, so the passes count `clipped` as they go.
//
// Zeros are no candidates (the rank is over lit counters), so the one value most of a Buddhabrot canvas holds never
// reaches the bins.  What is left still crowds: in the first digit pass nearly every lit counter has the same high byte,
// in the later ones nearly none has the prefix.  The adds are therefore aggregated per wave first (the lanes that share the
// first active lane's bin add once, by popcount: color.hip's scheme), the rest are LDS atomics on block-private u32 bins,
// flushed with one device-scope u64 atomic per non-empty bin per block.
//
// A u32 bin cannot overflow: a block counts at most the counters it reads, ceil(n / sweep) of its kBlockSweep-counter
// turns, and n <= kMaxCounters = 2^40 is enforced, so with the grid's cap of kExposureBlocks that is below 2^31.

#include "color_math.h"
#include "kernels.h"

namespace cb {

namespace {

constexpr uint32_t kExposureThreads = 256;
constexpr uint32_t kExposureBlocks = 1024;  // the grid's cap: four blocks per CU
constexpr uint32_t kVector = 2;             // counters per 16-byte load
constexpr uint32_t kLoads = 4;              // loads a lane has in flight
constexpr unsigned long long kBlockSweep = (unsigned long long) kExposureThreads * kLoads * kVector;  // counters per turn
constexpr unsigned long long kMaxCounters = 1ull << 40;
static_assert(kMaxCounters / kExposureBlocks + kBlockSweep < (1ull << 31), "a block's u32 bins hold what it reads");

// Every counter of hist[0, n) once, to f -- zero for the slots past the end.  f is called by every lane of the block the
// same number of times (the loop bounds are the block's), so it may ballot.  hist is 8-byte aligned; where it is not
// 16-byte aligned its first counter is taken apart, and so is a last one without a partner: the 16-byte loads are aligned
// and stay inside the buffer.  The two ends go to lanes 0 and 1 of block 0.
template <class F>
__device__ __forceinline__ void for_each_counter(const unsigned long long *hist, unsigned long long n, F f) {
  const unsigned long long head = (reinterpret_cast<uintptr_t>(hist) & 8u) ? 1ull : 0ull;  // n >= 1
  const ulonglong2 *vec = reinterpret_cast<const ulonglong2 *>(hist + head);
  const unsigned long long pairs = (n - head) / kVector;
  constexpr unsigned long long kTurn = (unsigned long long) kExposureThreads * kLoads;  // pairs a block takes per turn
  for (unsigned long long base = (unsigned long long) blockIdx.x * kTurn; base < pairs;
       base += (unsigned long long) gridDim.x * kTurn) {
    ulonglong2 q[kLoads];
#pragma unroll
    for (uint32_t j = 0; j < kLoads; ++j) {
      const unsigned long long at = base + (unsigned long long) j * kExposureThreads + threadIdx.x;
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

// Pass 0: out[0] = the largest counter, out[1] = the number of lit ones.
__global__ void __launch_bounds__(kExposureThreads) exposure_max_lit_kernel(const unsigned long long *hist,
                                                                            unsigned long long n,
                                                                            unsigned long long *out) {
  __shared__ unsigned long long wave_max[kExposureThreads / 64], wave_lit[kExposureThreads / 64];
  unsigned long long m = 0, lit = 0;
  for_each_counter(hist, n, [&](unsigned long long c) {
    m = c > m ? c : m;
    lit += c != 0ull ? 1ull : 0ull;
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
    lit += __shfl_xor(lit, d, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    wave_max[threadIdx.x >> 6] = m;
    wave_lit[threadIdx.x >> 6] = lit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < kExposureThreads / 64; ++k) {
      m = wave_max[k] > m ? wave_max[k] : m;
      lit += wave_lit[k];
    }
    if (lit != 0ull) {
      __hip_atomic_fetch_max(&out[0], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&out[1], lit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Lanes with `active` add 1 to lds[bin].  Every lane of the wave takes part (for_each_counter keeps it converged).
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

// A digit pass: bins[(c >> shift) & 255] over the lit counters c whose bits above the digit equal `prefix`.  The bits
// above are (c >> shift) >> 8: shift is at most 56, so the top digit's pass shifts by 56 and by 8, never by 64.
__global__ void __launch_bounds__(kExposureThreads) exposure_digit_kernel(const unsigned long long *hist,
                                                                          unsigned long long n,
                                                                          unsigned long long prefix, uint32_t shift,
                                                                          unsigned long long *bins) {
  __shared__ uint32_t lds[256];
  lds[threadIdx.x] = 0;
  __syncthreads();
  for_each_counter(hist, n, [&](unsigned long long c) {
    const unsigned long long from_digit = c >> shift;
    wave_count(lds, (uint32_t) from_digit & 255u, c != 0ull && (from_digit >> 8) == prefix);
  });
  __syncthreads();
  const uint32_t mine = lds[threadIdx.x];
  if (mine) {
    __hip_atomic_fetch_add(&bins[threadIdx.x], (unsigned long long) mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
static_assert(kExposureThreads == 256, "one lane per bin");

uint32_t exposure_grid(unsigned long long n) {
  const unsigned long long blocks = (n + kBlockSweep - 1) / kBlockSweep;
  return (uint32_t) (blocks == 0 ? 1 : (blocks > kExposureBlocks ? kExposureBlocks : blocks));
}

#define CB_EXPOSURE_TRY(expr)               \
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

}  // namespace

int white_count_device(const unsigned long long *hist, unsigned long long n, double clip_percent, uint64_t *white_out,
                       uint64_t *lit_out, uint64_t *clipped_out, uint64_t *max_out, hipStream_t stream) {
  if (!hist || (reinterpret_cast<uintptr_t>(hist) & 7u) != 0u || n == 0 || n > kMaxCounters || !white_out || !lit_out ||
      !clipped_out || !cb_white_clip_ok(clip_percent)) {
    return (int) hipErrorInvalidValue;
  }
  // [0] the maximum, [1] lit, then 256 bins for each of the eight digits
  constexpr size_t kWords = 2 + 8 * 256;
  DeviceBuffer work;
  CB_EXPOSURE_TRY(hipMalloc(&work.p, kWords * sizeof(unsigned long long)));
  unsigned long long *d_work = static_cast<unsigned long long *>(work.p);
  CB_EXPOSURE_TRY(hipMemsetAsync(d_work, 0, kWords * sizeof(unsigned long long), stream));
  const dim3 grid(exposure_grid(n)), block(kExposureThreads);
  hipLaunchKernelGGL(exposure_max_lit_kernel, grid, block, 0, stream, hist, n, d_work);
  CB_EXPOSURE_TRY(hipGetLastError());
  uint64_t max_lit[2] = {0, 0};
  CB_EXPOSURE_TRY(hipMemcpyAsync(max_lit, d_work, sizeof(max_lit), hipMemcpyDeviceToHost, stream));
  CB_EXPOSURE_TRY(hipStreamSynchronize(stream));
  const uint64_t max = max_lit[0], lit = max_lit[1];
  if (max_out) *max_out = max;
  *lit_out = lit;

  uint64_t rank = cb_white_rank(lit, clip_percent), white = max, clipped = 0;  // rank 0: the maximum (0 where nothing is lit)
  if (rank > 0) {
    int digits = 1;
    while (digits < 8 && (max >> (8 * digits)) != 0) ++digits;
    uint64_t prefix = 0, bins[256];
    for (int d = digits - 1; d >= 0; --d) {
      unsigned long long *d_bins = d_work + 2 + 256 * d;
      hipLaunchKernelGGL(exposure_digit_kernel, grid, block, 0, stream, hist, n, (unsigned long long) prefix,
                         (uint32_t) (8 * d), d_bins);
      CB_EXPOSURE_TRY(hipGetLastError());
      CB_EXPOSURE_TRY(hipMemcpyAsync(bins, d_bins, sizeof(bins), hipMemcpyDeviceToHost, stream));
      CB_EXPOSURE_TRY(hipStreamSynchronize(stream));
      uint64_t above = 0;  // the candidates with a larger digit: all above white
      const uint32_t k = color_select_high(bins, 256, rank, &above);
      rank -= above;
      clipped += above;
      prefix = (prefix << 8) | k;
    }
    white = prefix;
  }
  *white_out = white;
  *clipped_out = clipped;
  return 0;
}

int tone_map_white(const unsigned long long *hist, int w, int h, double gamma, int mode, double clip_percent,
                   uint16_t *d_gray_be, WhitePoint *found, hipStream_t stream) {
  if (!hist || !d_gray_be || !found || w <= 0 || h <= 0) return (int) hipErrorInvalidValue;
  if (mode != CB_TONE_AUTO && mode != CB_TONE_LUT && mode != CB_TONE_THRESHOLDS) return (int) hipErrorInvalidValue;
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h;
  const int rc = white_count_device(hist, n, clip_percent, &found->white, &found->lit, &found->clipped, &found->max, stream);
  if (rc) return rc;
  // the table or the thresholds over [0, white]: chosen by white, not by the maximum
  return tone_map_against(hist, n, found->white, found->max > found->white, gamma, mode, d_gray_be, stream);
}

}  // namespace cb

extern "C" int cb_white_count_device(const cb_pixel *d_hist, uint64_t n, double clip_percent, uint64_t *white_out,
                                     uint64_t *lit_out, uint64_t *clipped_out, void *stream) {
  return cb::white_count_device(reinterpret_cast<const unsigned long long *>(d_hist), n, clip_percent, white_out, lit_out,
                                clipped_out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int cb_tone_map_device_white(const cb_pixel *d_hist, int w, int h, double gamma, int mode, double clip_percent,
                                        uint16_t *d_gray_be, uint64_t *max_out, double *scale_out, uint64_t *white_out,
                                        void *stream) {
  cb::WhitePoint found = {0, 0, 0, 0};
  const int rc = cb::tone_map_white(reinterpret_cast<const unsigned long long *>(d_hist), w, h, gamma, mode, clip_percent,
                                    d_gray_be, &found, static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.white);
  if (white_out) *white_out = found.white;
  return 0;
}
