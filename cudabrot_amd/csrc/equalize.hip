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
// kWindow = 8192: 32 KB of LDS, four blocks per CU, which is all the grid's cap of kSweepBlocks ever asks for.
//
// The sweep is counter_sweep.h's, with the bound that keeps a u32 bin from overflowing.  The count below is the windowed
// form of that header's wave_count, kept apart: one vote primitive for both changes what the compiler makes of either.

#include <vector>

#include "counter_sweep.h"

namespace cb {

namespace {

constexpr uint32_t kWindow = 8192;  // keys below it are counted in LDS: counts below 2^17
static_assert(kWindow % 1024 == 0 && kWindow % kSweepThreads == 0 && kWindow <= CB_EQUALIZE_KEYS, "whole octaves");

// Lanes with `active` add 1 to the bin of `key`: in LDS below the window, in global memory from it on.  The lanes that
// share the first active lane's key add once.  Every lane of the wave takes part (for_each_counter keeps it converged).
__device__ __forceinline__ void window_count(uint32_t *lds, unsigned long long *bins, uint32_t key, bool active) {
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
__global__ void __launch_bounds__(kSweepThreads) equalize_bins_kernel(const unsigned long long *hist,
                                                                      unsigned long long n,
                                                                      unsigned long long *bins,
                                                                      unsigned long long *max) {
  __shared__ uint32_t lds[kWindow];
  __shared__ unsigned long long wave_max[kSweepThreads / 64];
  for (uint32_t k = threadIdx.x; k < kWindow; k += kSweepThreads) lds[k] = 0;
  __syncthreads();
  unsigned long long m = 0;
  for_each_counter(hist, n, [&](unsigned long long c) {
    m = c > m ? c : m;
    window_count(lds, bins, equalize_key(c), c != 0ull);
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kWindow; k += kSweepThreads) {
    const uint32_t mine = lds[k];
    if (mine) __hip_atomic_fetch_add(&bins[k], (unsigned long long) mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < kSweepThreads / 64; ++k) m = wave_max[k] > m ? wave_max[k] : m;
    if (m != 0ull) __hip_atomic_fetch_max(max, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// tonemap.hip's tone_lut_kernel, the index a key.  table has CB_EQUALIZE_KEYS entries.
__global__ void __launch_bounds__(kSweepThreads) equalize_map_kernel(const unsigned long long *hist,
                                                                     unsigned long long n, const uint16_t *table,
                                                                     uint16_t *out_be) {
  map_pairs(hist, n, out_be, [=](unsigned long long c) { return table[equalize_key(c)]; });
}

bool counters_ok(const unsigned long long *hist, unsigned long long n) {
  return hist && (reinterpret_cast<uintptr_t>(hist) & 7u) == 0u && n >= 1 && n <= kMaxCounters;
}

}  // namespace

int equalize_bins_device(const unsigned long long *hist, unsigned long long n, uint64_t *bins_out_host, uint64_t *lit_out,
                         uint64_t *max_out, hipStream_t stream) {
  if (!counters_ok(hist, n) || !bins_out_host || !lit_out || !max_out) return (int) hipErrorInvalidValue;
  constexpr size_t kWords = CB_EQUALIZE_KEYS + 1;  // the bins, then the maximum
  DeviceBuffer work;
  CB_HIP_TRY(hipMalloc(&work.p, kWords * sizeof(unsigned long long)));
  unsigned long long *d_work = static_cast<unsigned long long *>(work.p);
  CB_HIP_TRY(hipMemsetAsync(d_work, 0, kWords * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(equalize_bins_kernel, dim3(sweep_grid(n)), dim3(kSweepThreads), 0, stream, hist, n, d_work,
                     d_work + CB_EQUALIZE_KEYS);
  CB_HIP_TRY(hipGetLastError());
  std::vector<uint64_t> got(kWords);  // the caller's array is written only once everything has worked
  CB_HIP_TRY(hipMemcpyAsync(got.data(), d_work, kWords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));
  uint64_t lit = 0;
  for (size_t k = 0; k < CB_EQUALIZE_KEYS; ++k) {
    bins_out_host[k] = got[k];
    lit += got[k];
  }
  *lit_out = lit;
  *max_out = got[CB_EQUALIZE_KEYS];
  return 0;
}

int equalize_map_device(const unsigned long long *hist, unsigned long long n, const uint16_t *table_host, uint16_t *d_gray_be,
                        hipStream_t stream) {
  constexpr size_t kBytes = CB_EQUALIZE_KEYS * sizeof(uint16_t);
  DeviceBuffer d_table;
  CB_HIP_TRY(hipMalloc(&d_table.p, kBytes));
  CB_HIP_TRY(hipMemcpyAsync(d_table.p, table_host, kBytes, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(equalize_map_kernel, dim3(pairs_grid(n)), dim3(kSweepThreads), 0, stream, hist, n,
                     static_cast<const uint16_t *>(d_table.p), d_gray_be);
  CB_HIP_TRY(hipGetLastError());
  return (int) hipStreamSynchronize(stream);  // before the host table goes out of scope
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
  cb::Exposed found;
  const int rc = cb::tone_map_exposed(reinterpret_cast<const unsigned long long *>(d_hist), w, h, gamma, CB_TONE_AUTO,
                                      {cb::Exposure::kEqualized, 0.0}, d_gray_be, &found, static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.max);
  if (lit_out) *lit_out = found.lit;
  if (keys_out) *keys_out = found.keys;
  if (levels_out) *levels_out = found.levels;
  return 0;
}
