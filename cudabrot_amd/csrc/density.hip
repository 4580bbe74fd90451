// density.hip -- the density filter on the device (include/cudabrot_amd.h, "Density filter"): every
// counter spread with a binomial kernel whose radius falls as the count of its pixel rises, in u64 integers throughout.
//
// A gather, so that no two lanes ever add to one place and the result depends on no schedule: one workgroup per tile of
// kTileW x kTileH output pixels of one plane.
//   stage    the tile and a halo of R pixels around it, one 32-bit word per pixel: a counter that is smoothed is at most
//            T[1] < 2^22 and sits in the low 24 bits, its pixel's radius (1 .. 8) above them.  The key -- the sum over the
//            planes of the pixel's group -- and from it the radius are made as the word is loaded.  A pixel outside the
//            plane, a pixel with key 0 and a pixel of radius 0 stage the word 0: they spread nothing.
//   gather   each lane walks the neighbourhood of its pixel, as far as the largest radius staged in this block reaches
//            (0 in the dense parts of an image: no walk at all), and adds count * B_r[dy] * B_r[dx] * 2^(32 - 4r) of
//            every source in 64 bits: one 32 x 32 -> 64-bit multiply-add per tap, the weight the product of two table
//            entries, the row's carrying the shift.  A source whose radius does not reach the lane meets a zero entry.
//   finish   out = (sharp << 8) + (acc >> 24), sharp the lane's own counter where its pixel has radius 0.
// The counters are read and the results written 8 bytes per lane, lanes along a row: aligned whatever the plane's size.
//
// The refusal of a counter >= 2^55 is decided by a maximum pass in front (exposure.hip's sweep), before anything is written.

#include "counter_sweep.h"

namespace cb {

namespace {

constexpr uint32_t kTileW = 64;
constexpr uint32_t kTileH = 16;
constexpr uint32_t kDensityThreads = 256;
constexpr uint32_t kMaxR = CB_DENSITY_MAX_RADIUS;
constexpr uint32_t kHaloW = kTileW + 2 * kMaxR;  // the staged rows' stride; (kTileW + 2R) words of each are filled
constexpr uint32_t kHaloH = kTileH + 2 * kMaxR;
constexpr uint32_t kTaps = 2 * kMaxR + 1;        // a table row: offsets -8 .. 8
constexpr uint32_t kCountBits = 24;
constexpr uint32_t kRowsPerLane = kTileH * kTileW / kDensityThreads;
static_assert(kTileW == 64, "a wave is one row of the tile");
static_assert(kTileH % (kDensityThreads / kTileW) == 0, "every lane takes the same number of rows");
static_assert(CB_DENSITY_MAX_SMOOTHED <= (1ull << kCountBits) && kMaxR < (1u << (32 - kCountBits)), "count and radius share a word");
static_assert(kHaloW * kHaloH * sizeof(uint32_t) == 10240, "the staged tile is 10 KiB");

// [r][i + 8] = C(2r, i + r) for |i| <= r and r >= 1, else 0.
struct Binomials {
  uint32_t v[kMaxR + 1][kTaps];
};
constexpr Binomials make_binomials() {
  Binomials b = {};
  for (uint32_t r = 1; r <= kMaxR; ++r) {
    uint32_t row[2 * kMaxR + 1] = {1};
    for (uint32_t k = 1; k <= 2 * r; ++k) {
      for (uint32_t i = k; i >= 1; --i) row[i] += row[i - 1];
    }
    for (uint32_t i = 0; i <= 2 * r; ++i) b.v[r][i + kMaxR - r] = row[i];
  }
  return b;
}
__device__ const Binomials kBinomials = make_binomials();
static_assert(make_binomials().v[8][8] == 12870 && make_binomials().v[8][0] == 1 && make_binomials().v[4][8] == 70 &&
                  make_binomials().v[4][5] == 8 && make_binomials().v[4][3] == 0 && make_binomials().v[1][7] == 1 &&
                  make_binomials().v[1][6] == 0 && make_binomials().v[0][8] == 0,
              "C(16, 8), C(16, 0), C(8, 4), C(8, 1), and zeros past the edge of a kernel");

struct DensityArgs {
  const unsigned long long *in;
  unsigned long long *out;
  uint32_t w, h, group, radius;
  uint32_t thresholds[kMaxR + 1];  // T[1 .. R] (each < 2^22); 0 above R: no lit key is that small
};

__global__ void __launch_bounds__(kDensityThreads) density_filter_kernel(DensityArgs a) {
  __shared__ uint32_t tile[kHaloH * kHaloW];
  __shared__ uint32_t row_weight[(kMaxR + 1) * kTaps];  // B_r[i] << (32 - 4r): at most 2^(32 - 2r)
  __shared__ uint32_t col_weight[(kMaxR + 1) * kTaps];  // B_r[i]
  __shared__ uint32_t reach;                            // the largest radius staged
  const uint32_t tid = threadIdx.x;
  const uint32_t R = a.radius;
  const size_t plane_size = (size_t) a.w * (size_t) a.h;
  const size_t plane = blockIdx.z;
  const unsigned long long *in = a.in + plane * plane_size;
  const unsigned long long *first = a.in + (plane - plane % a.group) * plane_size;  // of the plane's group
  const long long x0 = (long long) blockIdx.x * kTileW, y0 = (long long) blockIdx.y * kTileH;

  if (tid < (kMaxR + 1) * kTaps) {
    const uint32_t r = tid / kTaps;
    const uint32_t b = kBinomials.v[r][tid % kTaps];
    row_weight[tid] = r == 0 ? 0u : b << (32u - 4u * r);
    col_weight[tid] = b;
  }
  if (tid == 0) reach = 0;
  __syncthreads();

  const uint32_t halo_w = kTileW + 2 * R, halo_h = kTileH + 2 * R;
  uint32_t longest = 0;
  for (uint32_t i = tid; i < halo_w * halo_h; i += kDensityThreads) {
    const uint32_t ty = i / halo_w, tx = i - ty * halo_w;
    const long long x = x0 - (long long) R + tx, y = y0 - (long long) R + ty;
    uint32_t word = 0;
    if (x >= 0 && x < (long long) a.w && y >= 0 && y < (long long) a.h) {
      const size_t at = (size_t) y * a.w + (size_t) x;
      const unsigned long long n = in[at];
      unsigned long long key = n;
      if (a.group == 3) key = first[at] + first[plane_size + at] + first[2 * plane_size + at];
      uint32_t r = 0;
#pragma unroll
      for (uint32_t k = 1; k <= kMaxR; ++k) r += key <= (unsigned long long) a.thresholds[k] ? 1u : 0u;
      if (key != 0ull && r != 0u) {  // n <= key <= T[1] < 2^22
        word = (uint32_t) n | (r << kCountBits);
        longest = r > longest ? r : longest;
      }
    }
    tile[ty * kHaloW + tx] = word;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t) __shfl_xor((int) longest, d, 64);
    longest = o > longest ? o : longest;
  }
  if ((tid & 63u) == 0u && longest != 0u) atomicMax(&reach, longest);
  __syncthreads();

  const int far = (int) reach;  // <= R: the walk stays inside what was staged
  const uint32_t lx = tid & (kTileW - 1);
  const long long x = x0 + lx;
  if (x >= (long long) a.w) return;
  for (uint32_t k = 0; k < kRowsPerLane; ++k) {
    const uint32_t ly = tid / kTileW + k * (kDensityThreads / kTileW);
    const long long y = y0 + ly;
    if (y >= (long long) a.h) return;
    const size_t at = (size_t) y * a.w + (size_t) x;
    const uint32_t centre = (ly + R) * kHaloW + lx + R;
    unsigned long long acc = 0;
    for (int dy = -far; dy <= far; ++dy) {
      for (int dx = -far; dx <= far; ++dx) {
        const uint32_t word = tile[(int) centre + dy * (int) kHaloW + dx];
        const uint32_t r = word >> kCountBits;
        const uint32_t weight = row_weight[r * kTaps + (uint32_t) (dy + (int) kMaxR)] *
                                col_weight[r * kTaps + (uint32_t) (dx + (int) kMaxR)];  // <= 2^30
        acc += (unsigned long long) (word & ((1u << kCountBits) - 1u)) * (unsigned long long) weight;
      }
    }
    const unsigned long long sharp = (tile[centre] >> kCountBits) == 0u ? in[at] : 0ull;  // (0 where the key is 0)
    a.out[plane * plane_size + at] = (sharp << 8) + (acc >> 24);
  }
}

}  // namespace

}  // namespace cb

extern "C" int cb_density_filter_device(const cb_pixel *d_hist, int w, int h, int planes, int group, int radius,
                                        const uint64_t *thresholds, uint64_t *d_out, void *stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!cb_density_arguments_ok(d_hist, w, h, planes, group, radius, thresholds, d_out)) return (int) hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(d_hist) | reinterpret_cast<uintptr_t>(d_out)) & 7u) != 0u) return (int) hipErrorInvalidValue;
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h * (unsigned long long) planes;
  const unsigned long long tiles_y = ((unsigned long long) h + cb::kTileH - 1) / cb::kTileH;
  if (n > cb::kMaxCounters || tiles_y > 65535ull || planes > 65535) return (int) hipErrorInvalidValue;  // (the grid's limits)
  // the largest counter, before anything is written
  uint64_t white = 0, lit = 0, clipped = 0, max = 0;
  const int rc = cb::white_count_device(reinterpret_cast<const unsigned long long *>(d_hist), n, 0.0, &white, &lit, &clipped,
                                        &max, stream);
  if (rc) return rc;
  if (max >= CB_DENSITY_MAX_COUNT) return (int) hipErrorInvalidValue;
  cb::DensityArgs a = {};
  a.in = reinterpret_cast<const unsigned long long *>(d_hist);
  a.out = reinterpret_cast<unsigned long long *>(d_out);
  a.w = (uint32_t) w;
  a.h = (uint32_t) h;
  a.group = (uint32_t) group;
  a.radius = (uint32_t) radius;
  for (int r = 1; r <= radius; ++r) a.thresholds[r] = (uint32_t) thresholds[r];
  const dim3 grid(((uint32_t) w + cb::kTileW - 1) / cb::kTileW, (uint32_t) tiles_y, (uint32_t) planes);
  hipLaunchKernelGGL(cb::density_filter_kernel, grid, dim3(cb::kDensityThreads), 0, stream, a);
  CB_HIP_TRY(hipGetLastError());
  return (int) hipStreamSynchronize(stream);
}
