// color.hip -- the colour stage on the device (include/cudabrot_amd.h, "Colour image").
//
// Three histograms -> one big-endian 16-bit RGB image, with only the finished image leaving the device:
//   1. each plane is tone-mapped by cb_tone_map_device (the PGM's values, big-endian) into one padded buffer;
//   2. exact percentile levels by a two-pass radix select: a 256-bin histogram of v >> 8 per plane, the host picks
//      the high-byte bucket that holds each rank (color_select_low / _high, the functions of the host path), then a
//      256-bin histogram of v & 255 restricted to those two buckets gives the low byte.  A 65536-bin u32 LDS histogram
//      (256 KiB) would not fit a CU's 160 KiB; two 256-bin ones take 2 KiB;
//   3. one kernel stretches, composes and writes the PPM body, 6 bytes per pixel, 8 pixels per lane (three 16-byte
//      stores).
// Buddhabrot planes are mostly zeros, so one bin takes most of the increments: the histogram adds are aggregated per
// wave first (counter_sweep.h's wave_count), the rest are LDS atomics.
#include <stdlib.h>

#include "counter_sweep.h"

namespace cb {

namespace {

constexpr uint32_t kColorThreads = 256;
constexpr uint32_t kLevelBlocksPerPlane = 1024;
constexpr uint32_t kComposeBlocks = 4096;

__device__ __forceinline__ void flush_bins(const uint32_t *lds, unsigned long long *bins) {
  const uint32_t c = lds[threadIdx.x];
  if (c) __hip_atomic_fetch_add(&bins[threadIdx.x], (unsigned long long) c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Values k of group g (8 pixels) of a big-endian plane: one 16-byte load; the plane is padded to 64 pixels, so the
// last group reads inside the buffer (its pixels >= n are masked by the caller).
__device__ __forceinline__ uint4 load_group(const uint16_t *plane, unsigned long long g) {
  return *reinterpret_cast<const uint4 *>(plane + g * 8ull);
}

__device__ __forceinline__ uint32_t value_of(const uint4 &q, int k) {
  const uint32_t w = (k < 2) ? q.x : (k < 4) ? q.y : (k < 6) ? q.z : q.w;
  return color_swap16((k & 1) ? (w >> 16) : (w & 0xffffu));
}

// Pass 1: bins[plane][v >> 8] over every pixel; blockIdx.y = plane.
__global__ void __launch_bounds__(kColorThreads) color_coarse_kernel(const uint16_t *gray_be, unsigned long long stride,
                                                                     unsigned long long n, unsigned long long *bins) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint16_t *plane = gray_be + (unsigned long long) blockIdx.y * stride;
  const unsigned long long groups = (n + 7ull) / 8ull;
  // the loop bound is the block's, not the lane's: the wave stays converged for wave_count
  for (unsigned long long g0 = (unsigned long long) blockIdx.x * kColorThreads; g0 < groups;
       g0 += (unsigned long long) gridDim.x * kColorThreads) {
    const unsigned long long g = g0 + threadIdx.x;
    uint4 q = {0u, 0u, 0u, 0u};
    if (g < groups) q = load_group(plane, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) wave_count(hist, value_of(q, k) >> 8, g * 8ull + (unsigned long long) k < n);
  }
  __syncthreads();
  flush_bins(hist, bins + (unsigned long long) blockIdx.y * 256ull);
}

struct Buckets {
  uint32_t black[3], white[3];  // the high byte that holds each plane's black / white rank
};

// Pass 2: bins[plane][0][v & 255] over the pixels with v >> 8 == black bucket, bins[plane][1][...] likewise for white.
__global__ void __launch_bounds__(kColorThreads) color_fine_kernel(const uint16_t *gray_be, unsigned long long stride,
                                                                   unsigned long long n, Buckets buckets,
                                                                   unsigned long long *bins) {
  __shared__ uint32_t hist[2][256];
  hist[0][threadIdx.x] = 0;
  hist[1][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t pl = blockIdx.y;
  const uint32_t bb = pl == 0 ? buckets.black[0] : (pl == 1 ? buckets.black[1] : buckets.black[2]);
  const uint32_t wb = pl == 0 ? buckets.white[0] : (pl == 1 ? buckets.white[1] : buckets.white[2]);
  const uint16_t *plane = gray_be + (unsigned long long) pl * stride;
  const unsigned long long groups = (n + 7ull) / 8ull;
  for (unsigned long long g0 = (unsigned long long) blockIdx.x * kColorThreads; g0 < groups;
       g0 += (unsigned long long) gridDim.x * kColorThreads) {
    const unsigned long long g = g0 + threadIdx.x;
    uint4 q = {0u, 0u, 0u, 0u};
    if (g < groups) q = load_group(plane, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t v = value_of(q, k);
      const bool in = g * 8ull + (unsigned long long) k < n;
      wave_count(hist[0], v & 255u, in && (v >> 8) == bb);
      wave_count(hist[1], v & 255u, in && (v >> 8) == wb);
    }
  }
  __syncthreads();
  flush_bins(hist[0], bins + (unsigned long long) pl * 512ull);
  flush_bins(hist[1], bins + (unsigned long long) pl * 512ull + 256ull);
}

struct ComposeArgs {
  PlaneLevels level[3];
  double hue_shift;
  int compose;
};

__device__ __forceinline__ void put_sample(uint32_t (&words)[12], int at, uint32_t v_be) {
  // at = 3k + c in [0, 24): u16 `at` of the group's 48 bytes
  words[at >> 1] |= (at & 1) ? (v_be << 16) : v_be;
}

// Pass 3: 8 pixels per lane -> 24 big-endian u16 (48 bytes) at out_be + 24 g: three 16-byte stores when the group is
// whole and out_be is 16-byte aligned, else one 2-byte store per sample.
__global__ void __launch_bounds__(kColorThreads) color_compose_kernel(const uint16_t *gray_be, unsigned long long stride,
                                                                      unsigned long long n, ComposeArgs a,
                                                                      uint16_t *out_be) {
  const unsigned long long groups = (n + 7ull) / 8ull;
  const bool aligned = (reinterpret_cast<uintptr_t>(out_be) & 15u) == 0u;
  for (unsigned long long g = (unsigned long long) blockIdx.x * kColorThreads + threadIdx.x; g < groups;
       g += (unsigned long long) gridDim.x * kColorThreads) {
    const uint4 q0 = load_group(gray_be, g);
    const uint4 q1 = load_group(gray_be + stride, g);
    const uint4 q2 = load_group(gray_be + 2ull * stride, g);
    uint32_t words[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t rgb[3];
      color_compose(a.compose, a.hue_shift, color_stretch(value_of(q0, k), a.level[0]),
                    color_stretch(value_of(q1, k), a.level[1]), color_stretch(value_of(q2, k), a.level[2]), rgb);
#pragma unroll
      for (int c = 0; c < 3; ++c) put_sample(words, 3 * k + c, color_swap16(rgb[c]));
    }
    uint16_t *dst = out_be + g * 24ull;
    if (aligned && g * 8ull + 8ull <= n) {
      uint4 *d4 = reinterpret_cast<uint4 *>(dst);
      d4[0] = make_uint4(words[0], words[1], words[2], words[3]);
      d4[1] = make_uint4(words[4], words[5], words[6], words[7]);
      d4[2] = make_uint4(words[8], words[9], words[10], words[11]);
    } else {
      const unsigned long long left = n - g * 8ull;  // >= 1
      const int samples = (int) (left < 8ull ? left : 8ull) * 3;
#pragma unroll
      for (int at = 0; at < 24; ++at) {
        if (at < samples) dst[at] = (uint16_t) ((at & 1) ? (words[at >> 1] >> 16) : (words[at >> 1] & 0xffffu));
      }
    }
  }
}

uint32_t blocks_for(unsigned long long groups, uint32_t cap) {
  const unsigned long long b = (groups + kColorThreads - 1) / kColorThreads;
  return (uint32_t) (b == 0 ? 1 : (b > cap ? cap : b));
}

}  // namespace

}  // namespace cb

extern "C" int cb_compose_color_device(const cb_pixel *const d_hist[3], int w, int h, double gamma, int tone_mode,
                                       const cb_color_params *p, uint16_t *d_rgb_be, uint16_t levels[6],
                                       void *stream_v) {
  using namespace cb;
  if (!d_hist || !d_hist[0] || !d_hist[1] || !d_hist[2] || !d_rgb_be || w <= 0 || h <= 0 || !color_params_ok(p)) {
    return (int) hipErrorInvalidValue;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h;
  const unsigned long long stride = (n + 63ull) & ~63ull;  // whole 16-byte groups, aligned planes
  const unsigned long long groups = (n + 7ull) / 8ull;
  DeviceBuffer gray, bins;
  CB_HIP_TRY(hipMalloc(&gray.p, 3ull * stride * sizeof(uint16_t)));
  uint16_t *d_gray = static_cast<uint16_t *>(gray.p);
  for (int j = 0; j < 3; ++j) {
    Exposed found;
    const int rc = tone_map_exposed(reinterpret_cast<const unsigned long long *>(d_hist[j]), w, h, gamma, tone_mode,
                                    {Exposure::kPlain, 0.0}, d_gray + (unsigned long long) j * stride, &found, stream);
    if (rc) return rc;
  }

  // levels: [3][256] high bytes, then [3][2][256] low bytes of the black and white buckets
  constexpr size_t kCoarse = 3 * 256, kFine = 3 * 2 * 256;
  CB_HIP_TRY(hipMalloc(&bins.p, (kCoarse + kFine) * sizeof(unsigned long long)));
  unsigned long long *d_coarse = static_cast<unsigned long long *>(bins.p);
  unsigned long long *d_fine = d_coarse + kCoarse;
  CB_HIP_TRY(hipMemsetAsync(bins.p, 0, (kCoarse + kFine) * sizeof(unsigned long long), stream));
  const dim3 level_grid(blocks_for(groups, kLevelBlocksPerPlane), 3);
  hipLaunchKernelGGL(color_coarse_kernel, level_grid, dim3(kColorThreads), 0, stream, d_gray, stride, n, d_coarse);
  CB_HIP_TRY(hipGetLastError());
  uint64_t coarse[kCoarse], fine[kFine];
  CB_HIP_TRY(hipMemcpyAsync(coarse, d_coarse, sizeof(coarse), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));

  uint64_t nb = 0, nw = 0;
  color_ranks(n, p, &nb, &nw);
  Buckets buckets;
  uint64_t black_rank[3], white_rank[3];  // the ranks left inside each bucket
  for (int j = 0; j < 3; ++j) {
    uint64_t below = 0, above = 0;
    buckets.black[j] = color_select_low(coarse + 256 * j, 256, nb, &below);
    buckets.white[j] = color_select_high(coarse + 256 * j, 256, nw, &above);
    black_rank[j] = nb - below;
    white_rank[j] = nw - above;
  }
  hipLaunchKernelGGL(color_fine_kernel, level_grid, dim3(kColorThreads), 0, stream, d_gray, stride, n, buckets, d_fine);
  CB_HIP_TRY(hipGetLastError());
  CB_HIP_TRY(hipMemcpyAsync(fine, d_fine, sizeof(fine), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));

  ComposeArgs a;
  a.compose = p->compose;
  a.hue_shift = p->hue_shift;
  for (int j = 0; j < 3; ++j) {
    uint64_t rest = 0;
    const uint32_t black = buckets.black[j] * 256u + color_select_low(fine + 512 * j, 256, black_rank[j], &rest);
    const uint32_t white = buckets.white[j] * 256u + color_select_high(fine + 512 * j + 256, 256, white_rank[j], &rest);
    a.level[j] = color_plane_levels(black, white);
    if (levels) {
      levels[2 * j] = (uint16_t) black;
      levels[2 * j + 1] = (uint16_t) white;
    }
  }
  hipLaunchKernelGGL(color_compose_kernel, dim3(blocks_for(groups, kComposeBlocks)), dim3(kColorThreads), 0, stream,
                     d_gray, stride, n, a, d_rgb_be);
  CB_HIP_TRY(hipGetLastError());
  CB_HIP_TRY(hipStreamSynchronize(stream));  // before the padded planes are freed
  return 0;
}
