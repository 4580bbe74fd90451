// equalize_local.hip -- the locally equalised image on the device (include/cudabrot_amd.h, "Locally equalised image";
// DESIGN.md 4.28): every tile of the canvas gets a rank curve of its own, and a pixel the blend of the four curves around it.
//
//   the maximum          tonemap.hip's hist_max_kernel, first: the image call needs it anyway, and its key bounds every
//                        per-tile array at K = key(max) + 1 entries -- the clear, the read-back and the tables that go up
//                        follow the lit key range (a few thousand keys), not all 56 320;
//   local_bins_kernel    one sweep of the u64 counters, tile by tile: bins[t][key(c)] over the lit counters of tile t;
//   the host             clips each tile's bins, tabulates them with cb_equalize_table's arithmetic, gives the empty tiles
//                        the global table (local_equalize_tables, host_output.cpp) and uploads TX * TY * K u16;
//   local_map_kernel     out[i] = big_endian(the blend of four table values at key(hist[i])), two pixels per lane; where
//                        a column and a row stand among the tile centres comes from two host-made tables (local_place,
//                        once per column and row: w + h entries of 16 bytes).
//
// A tile is swept by blocks_per_tile blocks, the grid about kSweepBlocks.  What a tile is made of is row segments, one per
// row of the tile and plane: a segment starts at (p * h + y) * w + ex[i], 16-byte aligned or not from row to row where w
// or ex[i] is odd.  So every segment is cut into slots -- a head counter, a tail counter, and the aligned pairs between
// them -- and a block's lanes take the slots of its share of the segments in turn, kLoads 16-byte loads in flight: the
// loads are aligned and stay inside the segment, and the loop bounds are the block's, so every ballot sees a whole wave.
//
// Crowding is what it is in equalize.hip, more so: a tile's lit counters sit in a few adjacent keys.  The count below is
// that file's window_count with the window a run-time value (K may lie below it), kept apart as the two of
// counter_sweep.h and equalize.hip are: one vote primitive for all changes what the compiler makes of each.

#include <vector>

#include "counter_sweep.h"
#include "equalize_local.h"

namespace cb {

namespace {

constexpr uint32_t kLocalWindow = 8192;  // keys below it are counted in LDS: counts below 2^17
static_assert(kLocalWindow % kSweepThreads == 0 && kLocalWindow <= CB_EQUALIZE_KEYS, "whole turns of the block");
constexpr unsigned long long kLocalMaxBlockCount = 0xffffffffull;  // counters a block may read: what a u32 LDS bin holds

// Lanes with `active` add 1 to the bin of `key`: in LDS below `window`, in the tile's global bins from it on (below n_keys:
// no key of the image is larger, and one that were is dropped, not written).  The lanes that share the first active lane's
// key add once.  Every lane of the wave takes part.
__device__ __forceinline__ void local_count(uint32_t *lds, unsigned long long *bins, uint32_t window, uint32_t n_keys,
                                            uint32_t key, bool active) {
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;
  const int first = __ffsll((long long) act) - 1;
  const uint32_t lead = (uint32_t) __builtin_amdgcn_readlane((int) key, first);
  const bool same = active && key == lead;
  const unsigned long long mate = __ballot(same);
  uint32_t add = active ? 1u : 0u;
  if (same) add = ((int) (threadIdx.x & 63u) == first) ? (uint32_t) __popcll(mate) : 0u;
  if (add != 0u) {
    if (key < window) {
      atomicAdd(&lds[key], add);
    } else if (key < n_keys) {
      __hip_atomic_fetch_add(&bins[key], (unsigned long long) add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// bins[t * n_keys + key(c)] over the lit counters of tile t.  Block b sweeps tile b / blocks_per_tile, and of every plane
// the tile's rows share, share + blocks_per_tile, ... with share = b % blocks_per_tile.
__global__ void __launch_bounds__(kSweepThreads) local_bins_kernel(const unsigned long long *hist, const LocalGrid *grid,
                                                                   uint32_t blocks_per_tile, uint32_t n_keys,
                                                                   unsigned long long *bins) {
  __shared__ uint32_t lds[kLocalWindow];
  const uint32_t window = n_keys < kLocalWindow ? n_keys : kLocalWindow;
  for (uint32_t k = threadIdx.x; k < window; k += kSweepThreads) lds[k] = 0;
  __syncthreads();
  const uint32_t tile = blockIdx.x / blocks_per_tile, share = blockIdx.x % blocks_per_tile;
  const uint32_t i = tile % grid->tx, j = tile / grid->tx;
  const uint32_t x0 = grid->ex[i], len = grid->ex[i + 1] - x0, y0 = grid->ey[j], rows = grid->ey[j + 1] - y0;
  const uint32_t w = grid->w, h = grid->h, planes = grid->planes;
  const uint32_t mine = rows > share ? (rows - share + blocks_per_tile - 1) / blocks_per_tile : 0;  // rows of a plane
  const uint32_t slots = len / 2 + 2;  // of a segment: its head, its tail, and room for every aligned pair
  const unsigned long long items = (unsigned long long) mine * slots;
  const unsigned long long odd = (reinterpret_cast<uintptr_t>(hist) & 8u) ? 1ull : 0ull;  // hist + e is aligned for e + odd even
  unsigned long long *tile_bins = bins + (unsigned long long) tile * n_keys;
  for (uint32_t p = 0; p < planes; ++p) {
    const unsigned long long first_row = (unsigned long long) p * h + y0 + share;
    for (unsigned long long base = 0; base < items; base += (unsigned long long) kSweepThreads * kLoads) {
      ulonglong2 q[kLoads];
#pragma unroll
      for (uint32_t l = 0; l < kLoads; ++l) {
        const unsigned long long item = base + (unsigned long long) l * kSweepThreads + threadIdx.x;
        q[l] = make_ulonglong2(0ull, 0ull);
        if (item < items) {
          const unsigned long long m = items <= 0xffffffffull ? (unsigned long long) ((uint32_t) item / slots) : item / slots;
          const uint32_t slot = (uint32_t) (item - m * slots);
          const unsigned long long begin = (first_row + m * blocks_per_tile) * w + x0, end = begin + len;
          const unsigned long long aligned = begin + ((begin + odd) & 1ull), pairs = (end - aligned) / 2ull;
          if (slot == 0u) {
            if (aligned > begin) q[l].x = hist[begin];
          } else if (slot == 1u) {
            if (aligned + 2ull * pairs < end) q[l].x = hist[end - 1ull];
          } else if (slot - 2u < pairs) {
            q[l] = *reinterpret_cast<const ulonglong2 *>(hist + aligned + 2ull * (slot - 2u));
          }
        }
      }
#pragma unroll
      for (uint32_t l = 0; l < kLoads; ++l) {
        local_count(lds, tile_bins, window, n_keys, equalize_key(q[l].x), q[l].x != 0ull);
        local_count(lds, tile_bins, window, n_keys, equalize_key(q[l].y), q[l].y != 0ull);
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < window; k += kSweepThreads) {
    const uint32_t counted = lds[k];
    if (counted) __hip_atomic_fetch_add(&tile_bins[k], (unsigned long long) counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The pixel of counter c in column x and row y: four table reads and the integer blend (equalize_local.h); the one division
// by dx * dy is a plain u64 divide, which is the definition's quotient.  A pixel that takes one tile alone (dx = dy = 1:
// outside the outermost centres of both axes) is that tile's table value, which is what the blend gives.
__device__ __forceinline__ uint32_t local_value(unsigned long long c, const LocalPlace &col, const LocalPlace &row, uint32_t tx,
                                                uint32_t n_keys, const uint16_t *tables) {
  if (c == 0ull) return 0u;  // every table has table[0] = 0
  uint32_t k = equalize_key(c);
  k = k < n_keys ? k : n_keys - 1u;  // (no key of the image is larger)
  const uint16_t *upper = tables + (size_t) row.i0 * tx * n_keys + k, *lower = tables + (size_t) row.i1 * tx * n_keys + k;
  const size_t left = (size_t) col.i0 * n_keys, right = (size_t) col.i1 * n_keys;
  if (col.d == 1u && row.d == 1u) return upper[left];
  return local_blend(upper[left], upper[right], lower[left], lower[right], col, row);
}

// map_pairs' shape (counter_sweep.h), the value a function of the place as well: two pixels per lane, one 4-byte store.
// The second pixel of a pair is the next of its row, or where w is odd the first of the next row.  places: local_place of
// every column, then of every row.
__global__ void __launch_bounds__(kSweepThreads) local_map_kernel(const unsigned long long *hist, unsigned long long n,
                                                                  const LocalGrid *grid, const LocalPlace *places,
                                                                  uint32_t n_keys, const uint16_t *tables, uint16_t *out_be) {
  const uint32_t w = grid->w, h = grid->h, tx = grid->tx;
  const LocalPlace *columns = places, *rows = places + w;
  const unsigned long long stride = (unsigned long long) gridDim.x * kSweepThreads * 2ull;
  for (unsigned long long i = ((unsigned long long) blockIdx.x * kSweepThreads + threadIdx.x) * 2ull; i < n; i += stride) {
    const unsigned long long line = i / w;
    uint32_t x = (uint32_t) (i - line * w), y = (uint32_t) (line % h);
    const uint32_t a = color_swap16(local_value(hist[i], columns[x], rows[y], tx, n_keys, tables));
    if (i + 1 < n) {
      if (++x == w) {
        x = 0;
        y = y + 1u == h ? 0u : y + 1u;
      }
      const uint32_t b = color_swap16(local_value(hist[i + 1], columns[x], rows[y], tx, n_keys, tables));
      *reinterpret_cast<uint32_t *>(out_be + i) = a | (b << 16);  // n even or not: i is even
    } else {
      out_be[i] = (uint16_t) a;
    }
  }
}

}  // namespace

// The bins of the tiles (bins_out_host: tx * ty rows of CB_EQUALIZE_KEYS, or null), the image (d_gray_be, or null), and
// what was found.  Nothing is written unless everything has worked.
int local_equalize_device(const unsigned long long *hist, int w, int h, int planes, int tx, int ty, uint32_t clip_q,
                          double gamma, uint64_t *bins_out_host, uint16_t *d_gray_be, Exposed *found, hipStream_t stream) {
  if (!hist || (reinterpret_cast<uintptr_t>(hist) & 7u) != 0u || !found || !cb_local_equalize_ok(w, h, planes, tx, ty, clip_q)) {
    return (int) hipErrorInvalidValue;
  }
  if ((reinterpret_cast<uintptr_t>(d_gray_be) & 3u) != 0u) return (int) hipErrorInvalidValue;  // the map stores 4 bytes
  if ((unsigned long long) w * (unsigned long long) h > kMaxCounters / (unsigned long long) planes) return (int) hipErrorInvalidValue;
  const unsigned long long n = (unsigned long long) w * (unsigned long long) h * (unsigned long long) planes;
  const LocalGrid g = local_grid(w, h, planes, tx, ty);
  // A block's u32 bins hold what it reads: ceil(rows / blocks_per_tile) segments of EVERY plane, none longer than len.  A
  // block sweeps all planes of its rows, so no number of blocks brings that below planes * len: a canvas whose widest
  // tile row, over all planes, does not fit a u32 is refused, before anything is read.  Below that, doubling the blocks
  // ends at one row a block at the latest.
  uint32_t blocks_per_tile = kSweepBlocks / (g.tx * g.ty), rows = 0, len = 0;
  for (uint32_t i = 0; i < g.tx; ++i) len = g.ex[i + 1] - g.ex[i] > len ? g.ex[i + 1] - g.ex[i] : len;
  for (uint32_t j = 0; j < g.ty; ++j) rows = g.ey[j + 1] - g.ey[j] > rows ? g.ey[j + 1] - g.ey[j] : rows;
  if ((unsigned long long) g.planes * len > kLocalMaxBlockCount) return (int) hipErrorInvalidValue;
  while ((unsigned long long) ((rows + blocks_per_tile - 1) / blocks_per_tile) * g.planes * len > kLocalMaxBlockCount) {
    blocks_per_tile *= 2;  // (below 2 * rows: one row a block satisfies the bound)
  }
  Exposed e = {0, 0, 0, 0, 0, 0};
  {
    const int rc = hist_max_device(hist, n, &e.max, stream);
    if (rc) return rc;
  }
  const uint32_t n_keys = equalize_key(e.max) + 1u, tiles = g.tx * g.ty;
  constexpr size_t kHead = 512;  // the grid, then the bins
  static_assert(sizeof(LocalGrid) <= kHead, "the grid fits its place");
  const size_t bin_words = (size_t) tiles * n_keys;
  DeviceBuffer work, d_tables, d_places;
  CB_HIP_TRY(hipMalloc(&work.p, kHead + bin_words * sizeof(unsigned long long)));
  const LocalGrid *d_grid = static_cast<const LocalGrid *>(work.p);
  unsigned long long *d_bins = reinterpret_cast<unsigned long long *>(static_cast<char *>(work.p) + kHead);
  CB_HIP_TRY(hipMemcpyAsync(work.p, &g, sizeof(g), hipMemcpyHostToDevice, stream));
  CB_HIP_TRY(hipMemsetAsync(d_bins, 0, bin_words * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(local_bins_kernel, dim3(tiles * blocks_per_tile), dim3(kSweepThreads), 0, stream, hist, d_grid,
                     blocks_per_tile, n_keys, d_bins);
  CB_HIP_TRY(hipGetLastError());
  std::vector<uint64_t> bins(bin_words);
  CB_HIP_TRY(hipMemcpyAsync(bins.data(), d_bins, bin_words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  CB_HIP_TRY(hipStreamSynchronize(stream));
  std::vector<uint16_t> tables(bin_words);
  local_equalize_tables(bins.data(), n_keys, tiles, clip_q, gamma, tables.data(), &e.lit, &e.lit_tiles, &e.moved);
  if (d_gray_be) {
    std::vector<LocalPlace> places((size_t) g.w + g.h);  // of every column, then of every row
    for (uint32_t x = 0; x < g.w; ++x) places[x] = local_place(g.cx, g.tx, 2u * x + 1u);
    for (uint32_t y = 0; y < g.h; ++y) places[(size_t) g.w + y] = local_place(g.cy, g.ty, 2u * y + 1u);
    CB_HIP_TRY(hipMalloc(&d_places.p, places.size() * sizeof(LocalPlace)));
    CB_HIP_TRY(hipMemcpyAsync(d_places.p, places.data(), places.size() * sizeof(LocalPlace), hipMemcpyHostToDevice, stream));
    CB_HIP_TRY(hipMalloc(&d_tables.p, bin_words * sizeof(uint16_t)));
    CB_HIP_TRY(hipMemcpyAsync(d_tables.p, tables.data(), bin_words * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(local_map_kernel, dim3(pairs_grid(n)), dim3(kSweepThreads), 0, stream, hist, n, d_grid,
                       static_cast<const LocalPlace *>(d_places.p), n_keys, static_cast<const uint16_t *>(d_tables.p), d_gray_be);
    CB_HIP_TRY(hipGetLastError());
    CB_HIP_TRY(hipStreamSynchronize(stream));  // before the host tables and places go out of scope
  }
  if (bins_out_host) {
    for (uint32_t t = 0; t < tiles; ++t) {
      uint64_t *row = bins_out_host + (size_t) t * CB_EQUALIZE_KEYS;
      for (uint32_t k = 0; k < CB_EQUALIZE_KEYS; ++k) row[k] = k < n_keys ? bins[(size_t) t * n_keys + k] : 0;
    }
  }
  *found = e;
  return 0;
}

}  // namespace cb

extern "C" int cb_local_equalize_bins_device(const cb_pixel *d_hist, int w, int h, int planes, int tx, int ty,
                                             uint64_t *bins_out_host, uint64_t *lit_out, uint64_t *max_out, void *stream) {
  if (!bins_out_host || !lit_out || !max_out) return (int) hipErrorInvalidValue;
  cb::Exposed found;
  const int rc = cb::local_equalize_device(reinterpret_cast<const unsigned long long *>(d_hist), w, h, planes, tx, ty, 0, 1.0,
                                           bins_out_host, nullptr, &found, static_cast<hipStream_t>(stream));
  if (rc) return rc;
  *lit_out = found.lit;
  *max_out = found.max;
  return 0;
}

extern "C" int cb_tone_map_device_local_equalized(const cb_pixel *d_hist, int w, int h, int planes, int tx, int ty,
                                                  uint32_t clip_q, double gamma, uint16_t *d_gray_be, uint64_t *max_out,
                                                  double *scale_out, uint64_t *lit_out, uint64_t *lit_tiles_out,
                                                  uint64_t *moved_out, void *stream) {
  if (!d_gray_be) return (int) hipErrorInvalidValue;
  cb::Exposed found;
  const int rc = cb::local_equalize_device(reinterpret_cast<const unsigned long long *>(d_hist), w, h, planes, tx, ty, clip_q,
                                           gamma, nullptr, d_gray_be, &found, static_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (max_out) *max_out = found.max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) found.max);
  if (lit_out) *lit_out = found.lit;
  if (lit_tiles_out) *lit_tiles_out = found.lit_tiles;
  if (moved_out) *moved_out = found.moved;
  return 0;
}
