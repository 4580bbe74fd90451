// equalize.hip -- the equalised image on the device (include/cudabrot_amd.h, "Equalised image"): a pixel's
// value is the rank of its counter among the lit ones, through cb_tone_value.
//
//   equalize_bins_kernel  one streaming sweep of the u64 counters: bins[key(c)] over the lit ones, CB_EQUALIZE_KEYS u64
//                         bins in global memory (440 KB), and the largest counter beside them (a compare per counter in
//                         the same sweep: no second pass);
//   the host              prefix-sums the bins and evaluates the table with cb_tone_value (cb_equalize_table: the only
//                         floating point, one pow per lit key), 110 KB that go back up;
//   equalize_map_kernel   out[i] = big_endian(table[key(hist[i])]), the table read from global memory.
//
// Crowding decides the first kernel: a render's lit counters sit in a few hundred adjacent keys, an all-ones histogram in
// one.  exposure.hip's scheme, widened: the lanes of a wave that share the first active lane's key add once, by popcount;
// keys below kWindow go to block-private u32 bins in LDS, flushed with one device-scope u64 atomic per non-empty bin per
// block; keys at or above it -- counts of 2^17 and more, the few hot pixels of an image -- go to the global bins directly.
// kWindow = 8192: 32 KB of LDS, four blocks per CU, which is all the grid's cap of kEqualizeBlocks ever asks for.
//
// A u32 bin cannot overflow: a block counts at most the counters it reads, and n <= kMaxCounters = 2^40 is enforced.
//
// for_each_counter is exposure.hip's, restated: that file's kernels and their record are pinned.

#include <vector>

#include "color_math.h"
#include "kernels.h"

namespace cb {

namespace {

constexpr uint32_t kEqualizeThreads = 256;
constexpr uint32_t kEqualizeBlocks = 1024;  // the grid's cap: four blocks per CU
constexpr uint32_t kVector = 2;             // counters per 16-byte load
constexpr uint32_t kLoads = 4;              // loads a lane has in flight
constexpr uint32_t kWindow = 8192;          // keys below it are counted in LDS: counts below 2^17
constexpr unsigned long long kBlockSweep = (unsigned long long) kEqualizeThreads * kLoads * kVector;  // counters per turn
constexpr unsigned long long kMaxCounters = 1ull << 40;
static_assert(kMaxCounters / kEqualizeBlocks + kBlockSweep < (1ull << 31), "a block's u32 bins hold what it reads");
static_assert(kWindow % 1024 == 0 && kWindow % kEqualizeThreads == 0 && kWindow <= CB_EQUALIZE_KEYS, "whole octaves");

// Every counter of hist[0, n) once, to f -- zero for the slots past the end.  f is called by every lane of the block the
// same number of times (the loop bounds are the block's), so it may ballot.  hist is 8-byte aligned; where it is not
// 16-byte aligned its first counter is taken apart, and so is a last one without a partner: the 16-byte loads are aligned
// and stay inside the buffer.  The two ends go to lanes 0 and 1 of block 0.
template <class F>
__device__ __forceinline__ void for_each_counter(const unsigned long long *hist, unsigned long long n, F f) {
  const unsigned long long head = (reinterpret_cast<uintptr_t>(hist) & 8u) ? 1ull : 0ull;  // n >= 1
  const ulonglong2 *vec = reinterpret_cast<const ulonglong2 *>(hist + head);
  const unsigned long long pairs = (n - head) / kVector;
  constexpr unsigned long long kTurn = (unsigned long long) kEqualizeThreads * kLoads;  // pairs a block takes per turn
  for (unsigned long long base = (unsigned long long) blockIdx.x * kTurn; base < pairs;
       base += (unsigned long long) gridDim.x * kTurn) {
    ulonglong2 q[kLoads];
#pragma unroll
    for (uint32_t j = 0; j < kLoads; ++j) {
      const unsigned long long at = base + (unsigned long long) j * kEqualizeThreads + threadIdx.x;
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

// Lanes with `active` add 1 to the bin of `key`: in LDS below the window, in global memory from it on.  The lanes that
// share the first active lane's key add once.  Every lane of the wave takes part (for_each_counter keeps it converged).
__device__ __forceinline__ void wave_count(uint32_t *lds, unsigned long long *bins, uint32_t key, bool active) {
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;
  const int first = __ffsll((long long) act) - 1;
  const uint32_t lead = (uint32_t) __builtin_amdgcn_readlane((int) key, first);
  const bool same = active && key == lead;
  const unsigned long long mate = __ballot(same);
  uint32_t add = active ? 1u : 0u;
  if (same) add = ((int) (threadIdx.x & 63u) == first) ? (uint32_t) __popcll(mate) : 0u;
  if (add != 0u) {
    if (key < kWindow) {
      atomicAdd(&lds[key], add);
    } else {
      __hip_atomic_fetch_add(&bins[key], (unsigned long long) add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// bins[key(c)] over the lit counters, and *max = the largest counter.  bins has CB_EQUALIZE_KEYS entries: a key is below
// that for every u64.
__global__ void __launch_bounds__(kEqualizeThreads) equalize_bins_kernel(const unsigned long long *hist,
                                                                         unsigned long long n,
                                                                         unsigned long long *bins,
                                                                         unsigned long long *max) {
  __shared__ uint32_t lds[kWindow];
  __shared__ unsigned long long wave_max[kEqualizeThreads / 64];
  for (uint32_t k = threadIdx.x; k < kWindow; k += kEqualizeThreads) lds[k] = 0;
  __syncthreads();
  unsigned long long m = 0;
  for_each_counter(hist, n, [&](unsigned long long c) {
    m = c > m ? c : m;
    wave_count(lds, bins, equalize_key(c), c != 0ull);
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kWindow; k += kEqualizeThreads) {
    const uint32_t mine = lds[k];
    if (mine) __hip_atomic_fetch_add(&bins[k], (unsigned long long) mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < kEqualizeThreads / 64; ++k) m = wave_max[k] > m ? wave_max[k] : m;
    if (m != 0ull) __hip_atomic_fetch_max(max, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// two pixels per lane: one 4-byte store (tonemap.hip's tone_lut_kernel, the index a key).  table has CB_EQUALIZE_KEYS
// entries.
__global__ void __launch_bounds__(kEqualizeThreads) equalize_map_kernel(const unsigned long long *hist,
                                                                        unsigned long long n, const uint16_t *table,
                                                                        uint16_t *out_be) {
  const unsigned long long stride = (unsigned long long) gridDim.x * kEqualizeThreads * 2ull;
  for (unsigned long long i = ((unsigned long long) blockIdx.x * kEqualizeThreads + threadIdx.x) * 2ull; i < n;
       i += stride) {
    const uint32_t a = color_swap16(table[equalize_key(hist[i])]);
    if (i + 1 < n) {
      const uint32_t b = color_swap16(table[equalize_key(hist[i + 1])]);
      *reinterpret_cast<uint32_t *>(out_be + i) = a | (b << 16);  // n even or not: i is even
    } else {
      out_be[i] = (uint16_t) a;
    }
  }
}

uint32_t bins_grid(unsigned long long n) {
  const unsigned long long blocks = (n + kBlockSweep - 1) / kBlockSweep;
  return (uint32_t) (blocks == 0 ? 1 : (blocks > kEqualizeBlocks ? kEqualizeBlocks : blocks));
}

uint32_t map_grid(unsigned long long n) {  // tonemap.hip's
  unsigned long long blocks = (n / 2 + kEqualizeThreads) / kEqualizeThreads;
  if (blocks > 256ull * 16ull) blocks = 256ull * 16ull;
  return (uint32_t) (blocks ? blocks : 1);
}

#define CB_EQUALIZE_TRY(expr)               \
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

bool counters_ok(const unsigned long long *hist, unsigned long long n) {
  return hist && (reinterpret_cast<uintptr_t>(hist) & 7u) == 0u && n >= 1 && n <= kMaxCounters;
}

}  // namespace

int equalize_bins_device(const unsigned long long *hist, unsigned long long n, uint64_t *bins_out_host, uint64_t *lit_out,
                         uint64_t *max_out, hipStream_t stream) {
  if (!counters_ok(hist, n) || !bins_out_host || !lit_out || !max_out) return (int) hipErrorInvalidValue;
  constexpr size_t kWords = CB_EQUALIZE_KEYS + 1;  // the bins, then the maximum
  DeviceBuffer work;
  CB_EQUALIZE_TRY(hipMalloc(&work.p, kWords * sizeof(unsigned long long)));
  unsigned long long *d_work = static_cast<unsigned long long *>(work.p);
  CB_EQUALIZE_TRY(hipMemsetAsync(d_work, 0, kWords * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(equalize_bins_kernel, dim3(bins_grid(n)), dim3(kEqualizeThreads), 0, stream, hist, n, d_work,
                     d_work + CB_EQUALIZE_KEYS);
  CB_EQUALIZE_TRY(hipGetLastError());
  std::vector<uint64_t> got(kWords);  // the caller's array is written only once everything has worked
  CB_EQUALIZE_TRY(hipMemcpyAsync(got.data(), d_work, kWords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  CB_EQUALIZE_TRY(hipStreamSynchronize(stream));
  uint64_t lit = 0;
  for (size_t k = 0; k < CB_EQUALIZE_KEYS; ++k) {
    bins_out_host[k] = got[k];
    lit += got[k];
  }
  *lit_out = lit;
  *max_out = got[CB_EQUALIZE_KEYS];
  return 0;
}

int tone_map_equalized(const unsigned long long *hist, int w, int h, double gamma, uint16_t *d_gray_be, Equalized *found,
                       hipStream_t stream) {
  if (!hist || !d_gray_be || !found || w <= 0 || h <= 0) return (int) hipErrorInvalidValue;
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h;
  std::vector<uint64_t> bins(CB_EQUALIZE_KEYS);
  std::vector<uint16_t> table(CB_EQUALIZE_KEYS);
  Equalized e = {0, 0, 0, 0};
  int rc = equalize_bins_device(hist, n, bins.data(), &e.lit, &e.max, stream);
  if (rc == 0) rc = cb_equalize_table(bins.data(), gamma, table.data(), &e.keys, &e.levels);
  if (rc) return rc;
  DeviceBuffer d_table;
  CB_EQUALIZE_TRY(hipMalloc(&d_table.p, table.size() * sizeof(uint16_t)));
  CB_EQUALIZE_TRY(hipMemcpyAsync(d_table.p, table.data(), table.size() * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(equalize_map_kernel, dim3(map_grid(n)), dim3(kEqualizeThreads), 0, stream, hist, n,
                     static_cast<const uint16_t *>(d_table.p), d_gray_be);
  CB_EQUALIZE_TRY(hipGetLastError());
  CB_EQUALIZE_TRY(hipStreamSynchronize(stream));  // before the host table goes out of scope
  *found = e;
  return 0;
}

}  // namespace cb

extern "C" int cb_equalize_bins_device(const cb_pixel *d_hist, uint64_t n, uint64_t *bins_out_host, uint64_t *lit_out,
                                       uint64_t *max_out, void *stream) {
  return cb::equalize_bins_device(reinterpret_cast<const unsigned long long *>(d_hist), n, bins_out_host, lit_out, max_out,
                                  static_cast<hipStream_t>(stream));
}

extern "C" int cb_tone_map_device_equalized(const cb_pixel *d_hist, int w, int h, double gamma, uint16_t *d_gray_be,
                                            uint64_t *max_out, double *scale_out, uint64_t *lit_out, uint64_t *keys_out,
                                            uint64_t *levels_out, void *stream) {
  cb::Equalized found = {0, 0, 0, 0};
  const int rc = cb::tone_map_equalized(reinterpret_cast<const unsigned long long *>(d_hist), w, h, gamma, d_gray_be, &found,
                                        static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.max);
  if (lit_out) *lit_out = found.lit;
  if (keys_out) *keys_out = found.keys;
  if (levels_out) *levels_out = found.levels;
  return 0;
}
