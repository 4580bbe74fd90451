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
// The sweep and the wave's count are counter_sweep.h's, with the bound that keeps a u32 bin from overflowing.

#include "counter_sweep.h"

namespace cb {

namespace {

// Pass 0: out[0] = the largest counter, out[1] = the number of lit ones.
__global__ void __launch_bounds__(kSweepThreads) exposure_max_lit_kernel(const unsigned long long *hist,
                                                                         unsigned long long n,
                                                                         unsigned long long *out) {
  __shared__ unsigned long long wave_max[kSweepThreads / 64], wave_lit[kSweepThreads / 64];
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
    for (uint32_t k = 1; k < kSweepThreads / 64; ++k) {
      m = wave_max[k] > m ? wave_max[k] : m;
      lit += wave_lit[k];
    }
    if (lit != 0ull) {
      __hip_atomic_fetch_max(&out[0], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&out[1], lit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// A digit pass: bins[(c >> shift) & 255] over the lit counters c whose bits above the digit equal `prefix`.  The bits
// above are (c >> shift) >> 8: shift is at most 56, so the top digit's pass shifts by 56 and by 8, never by 64.
__global__ void __launch_bounds__(kSweepThreads) exposure_digit_kernel(const unsigned long long *hist,
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
static_assert(kSweepThreads == 256, "one lane per bin");

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
  CB_HIP_TRY(hipMalloc(&work.p, kWords * sizeof(unsigned long long)));
  unsigned long long *d_work = static_cast<unsigned long long *>(work.p);
  CB_HIP_TRY(hipMemsetAsync(d_work, 0, kWords * sizeof(unsigned long long), stream));
  const dim3 grid(sweep_grid(n)), block(kSweepThreads);
  hipLaunchKernelGGL(exposure_max_lit_kernel, grid, block, 0, stream, hist, n, d_work);
  CB_HIP_TRY(hipGetLastError());
  uint64_t max_lit[2] = {0, 0};
  CB_HIP_TRY(hipMemcpyAsync(max_lit, d_work, sizeof(max_lit), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));
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
      CB_HIP_TRY(hipGetLastError());
      CB_HIP_TRY(hipMemcpyAsync(bins, d_bins, sizeof(bins), hipMemcpyDeviceToHost, stream));
      CB_HIP_TRY(hipStreamSynchronize(stream));
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

}  // namespace cb

extern "C" int cb_white_count_device(const cb_pixel *d_hist, uint64_t n, double clip_percent, uint64_t *white_out,
                                     uint64_t *lit_out, uint64_t *clipped_out, void *stream) {
  return cb::white_count_device(reinterpret_cast<const unsigned long long *>(d_hist), n, clip_percent, white_out, lit_out,
                                clipped_out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int cb_tone_map_device_white(const cb_pixel *d_hist, int w, int h, double gamma, int mode, double clip_percent,
                                        uint16_t *d_gray_be, uint64_t *max_out, double *scale_out, uint64_t *white_out,
                                        void *stream) {
  cb::Exposed found;
  const int rc = cb::tone_map_exposed(reinterpret_cast<const unsigned long long *>(d_hist), w, h, gamma, mode,
                                      {cb::Exposure::kWhiteClip, clip_percent}, d_gray_be, &found,
                                      static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.white);
  if (white_out) *white_out = found.white;
  return 0;
}
