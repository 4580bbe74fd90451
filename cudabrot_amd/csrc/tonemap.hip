// tonemap.hip -- the output stage on the device: SetGrayscalePixels
// (cudabrot.cu:425-468) and the byte swap of SaveImage (cudabrot.cu:566-570).
//
// The reference scans the histogram for its maximum, maps every pixel through
//   v = 65535 * pow(count * scale / 65535, 1 / gamma)          (cudabrot.cu:443-449)
// on one host thread and swaps the bytes of the result: at 20000 x 20000 that is a 3.2 GB copy to
// the host and tens of seconds of pow().  Here the histogram stays on the device; only 2 bytes per
// pixel, already big-endian, travel.
//
// Bit-exactness.  The value of a pixel depends on its count alone (and on max, gamma), and pow() of
// the host's libm and of the device library differ in the last place, which after the truncation to
// uint16 shows as off-by-one pixels.  So the HOST evaluates the map -- the same function
// cb_set_grayscale_pixels uses (cb_tone_value, host_output.cpp) -- and the device only looks it up:
//   CB_TONE_LUT         one uint16 per count in [0, max]: identical to the host path by construction
//   CB_TONE_THRESHOLDS  for every output value k the smallest count that reaches it (65535
//                       bisections over the host map); a pixel's value is the number of thresholds
//                       <= its count.  Identical whenever the host map is monotone in the count,
//                       which holds for a pow() that is within an ulp of exact; used when max is too
//                       large for a table (> 2^24).
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "counter_sweep.h"

extern "C" uint16_t cb_tone_value(uint64_t count, uint64_t max, double gamma);

namespace cb {

namespace {

constexpr uint64_t kLutMaxEntries = 1ull << 24;

__global__ void __launch_bounds__(kSweepThreads) hist_max_kernel(const unsigned long long *hist,
                                                                 unsigned long long n,
                                                                 unsigned long long *out) {
  unsigned long long m = 0;
  const unsigned long long stride = (unsigned long long) gridDim.x * kSweepThreads;
  for (unsigned long long i = (unsigned long long) blockIdx.x * kSweepThreads + threadIdx.x; i < n;
       i += stride) {
    const unsigned long long v = hist[i];
    m = v > m ? v : m;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0u && m != 0ull) {
    __hip_atomic_fetch_max(out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// kClamp (the white clip, exposure.hip): the table ends at `top` and every larger count reads its last entry; without it
// `top` is not read and the kernel is the one it was.
template <bool kClamp>
__global__ void __launch_bounds__(kSweepThreads) tone_lut_kernel(const unsigned long long *hist,
                                                                 unsigned long long n,
                                                                 const uint16_t *lut, unsigned long long top,
                                                                 uint16_t *out_be) {
  map_pairs(hist, n, out_be, [=](unsigned long long c) { return lut[kClamp ? (c < top ? c : top) : c]; });
}

// thr[k], k in [0, 65536): smallest count whose value is >= k (thr[0] = 0; ~0 if none).  The value
// of a count is the largest k with thr[k] <= count.
__device__ __forceinline__ uint32_t value_by_thresholds(unsigned long long c,
                                                        const unsigned long long *thr) {
  uint32_t lo = 0, hi = 65536;  // invariant: thr[lo] <= c, and (hi == 65536 or thr[hi] > c)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (thr[mid] <= c) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

__global__ void __launch_bounds__(kSweepThreads) tone_thresholds_kernel(const unsigned long long *hist,
                                                                        unsigned long long n,
                                                                        const unsigned long long *thr,
                                                                        uint16_t *out_be) {
  map_pairs(hist, n, out_be, [=](unsigned long long c) { return value_by_thresholds(c, thr); });
}

// thr[k] = smallest count in [0, max] whose value is >= k, by bisection over the host map
std::vector<unsigned long long> build_thresholds(unsigned long long max, double gamma) {
  std::vector<unsigned long long> thr(65536, ~0ull);
  thr[0] = 0;
  const uint32_t top = cb_tone_value(max, max, gamma);
  unsigned long long lo = 0;  // thr is non-decreasing: each search starts at the previous answer
  for (uint32_t k = 1; k <= top; ++k) {
    unsigned long long a = lo, b = max;  // value(max) = top >= k
    if (cb_tone_value(a, max, gamma) >= k) {
      b = a;
    } else {
      while (b - a > 1ull) {  // value(a) < k <= value(b)
        const unsigned long long mid = a + (b - a) / 2ull;
        if (cb_tone_value(mid, max, gamma) >= k) {
          b = mid;
        } else {
          a = mid;
        }
      }
    }
    thr[k] = b;
    lo = b;
  }
  return thr;
}

}  // namespace

// The largest of n device counters (GetLinearColorScale, cudabrot.cu:425-439).
int hist_max_device(const unsigned long long *hist, unsigned long long n, uint64_t *max_out, hipStream_t stream) {
  DeviceBuffer d_max;
  CB_HIP_TRY(hipMalloc(&d_max.p, sizeof(unsigned long long)));
  CB_HIP_TRY(hipMemsetAsync(d_max.p, 0, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(hist_max_kernel, dim3(pairs_grid(n)), dim3(kSweepThreads), 0, stream, hist, n,
                     static_cast<unsigned long long *>(d_max.p));
  CB_HIP_TRY(hipGetLastError());
  CB_HIP_TRY(hipMemcpyAsync(max_out, d_max.p, sizeof(*max_out), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

namespace {

// The map against `top` on a device histogram of n counters: the table over [0, top] or the thresholds, as `mode` and
// `top` choose.  clamp: counts above `top` exist (the white clip) and take top's value.
int tone_map_against(const unsigned long long *hist, unsigned long long n, unsigned long long top, bool clamp, double gamma,
                     int mode, uint16_t *d_gray_be, hipStream_t stream) {
  DeviceBuffer d_table;
  const dim3 grid(pairs_grid(n)), block(kSweepThreads);
  if (mode == CB_TONE_AUTO) mode = (top < kLutMaxEntries) ? CB_TONE_LUT : CB_TONE_THRESHOLDS;
  if (mode == CB_TONE_LUT) {
    if (top >= (1ull << 32)) return (int) hipErrorInvalidValue;  // not a sensible table
    std::vector<uint16_t> lut((size_t) top + 1);
    for (unsigned long long c = 0; c <= top; ++c) lut[(size_t) c] = cb_tone_value(c, top, gamma);
    CB_HIP_TRY(hipMalloc(&d_table.p, lut.size() * sizeof(uint16_t)));
    CB_HIP_TRY(hipMemcpyAsync(d_table.p, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
    const auto lut_kernel = clamp ? tone_lut_kernel<true> : tone_lut_kernel<false>;
    hipLaunchKernelGGL(lut_kernel, grid, block, 0, stream, hist, n, static_cast<const uint16_t *>(d_table.p), top, d_gray_be);
    CB_HIP_TRY(hipGetLastError());
    CB_HIP_TRY(hipStreamSynchronize(stream));  // before the host table goes out of scope
  } else {
    // No clamp here, with a white clip or without: thr[k] is the smallest count in [0, top] whose value reaches k, the
    // value of a count is the number of thresholds <= it, and every threshold is <= top -- so a count above top has
    // top's value already.
    const std::vector<unsigned long long> thr = build_thresholds(top, gamma);
    CB_HIP_TRY(hipMalloc(&d_table.p, thr.size() * sizeof(unsigned long long)));
    CB_HIP_TRY(hipMemcpyAsync(d_table.p, thr.data(), thr.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(tone_thresholds_kernel, grid, block, 0, stream, hist, n,
                       static_cast<const unsigned long long *>(d_table.p), d_gray_be);
    CB_HIP_TRY(hipGetLastError());
    CB_HIP_TRY(hipStreamSynchronize(stream));
  }
  return 0;
}

}  // namespace

// Find, map, report.  The find step is the kind's own: hist_max_kernel; the radix select of exposure.hip; the bins of
// equalize.hip and the host's table of them; the bins of the tiles, equalize_local.hip's.  Under a white clip the table
// or the thresholds are chosen by white, not by the maximum.
int tone_map_exposed(const unsigned long long *hist, int w, int h, double gamma, int mode, const Exposure &how,
                     uint16_t *d_gray_be, Exposed *found, hipStream_t stream) {
  if (!hist || !d_gray_be || !found || w <= 0 || h <= 0 || !tone_mode_ok(mode)) return (int) hipErrorInvalidValue;
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h;
  Exposed e = {0, 0, 0, 0, 0, 0};
  int rc;
  if (how.kind == Exposure::kLocalEqualized) {  // h rows: `planes` planes of h / planes rows
    if (how.planes < 1 || h % how.planes != 0) return (int) hipErrorInvalidValue;
    rc = local_equalize_device(hist, w, h / how.planes, how.planes, how.tiles_x, how.tiles_y, how.clip_q, gamma, nullptr,
                               d_gray_be, &e, stream);
  } else if (how.kind == Exposure::kEqualized) {
    std::vector<uint64_t> bins(CB_EQUALIZE_KEYS);
    std::vector<uint16_t> table(CB_EQUALIZE_KEYS);
    rc = equalize_bins_device(hist, n, bins.data(), &e.lit, &e.max, stream);
    if (rc == 0) rc = cb_equalize_table(bins.data(), gamma, table.data(), &e.keys, &e.levels);
    if (rc == 0) rc = equalize_map_device(hist, n, table.data(), d_gray_be, stream);
  } else if (how.kind == Exposure::kWhiteClip) {
    rc = white_count_device(hist, n, how.clip_percent, &e.white, &e.lit, &e.clipped, &e.max, stream);
    if (rc == 0) rc = tone_map_against(hist, n, e.white, e.max > e.white, gamma, mode, d_gray_be, stream);
  } else {
    rc = hist_max_device(hist, n, &e.max, stream);
    if (rc == 0) rc = tone_map_against(hist, n, e.max, false, gamma, mode, d_gray_be, stream);
  }
  if (rc == 0) *found = e;
  return rc;
}

}  // namespace cb

extern "C" int cb_tone_map_device(const cb_pixel *d_hist, int w, int h, double gamma, int mode,
                                  uint16_t *d_gray_be, uint64_t *max_out, double *scale_out,
                                  void *stream) {
  cb::Exposed found;
  const int rc = cb::tone_map_exposed(reinterpret_cast<const unsigned long long *>(d_hist), w, h, gamma, mode,
                                      {cb::Exposure::kPlain, 0.0}, d_gray_be, &found, static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.max);
  return 0;
}

