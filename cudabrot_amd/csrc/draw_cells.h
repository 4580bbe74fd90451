// draw_cells.h -- the cell grid of the sample plane (include/cudabrot_amd.h, "Focused render"), for the
// kernels that draw their samples from a list of its cells or mark the cells their samples lie in (draw_focus.hip,
// draw_aim.hip).  Grid is the block that holds the grid's members -- FocusArgs' CellGrid, or AimArgs itself (kernels.h) -- in
// whatever address space the caller reads it from: a copy of the kernel's argument, or the argument itself (draw_aim.hip,
// fresh_aim_args).
#pragma once

#include "draw_rounds.h"

namespace cb {

namespace {

// The next sample of a thread.  Uniform source: two coordinates, two draws each.  Cell list: a, b -> entry
// j = high half of (a << 32 | b) * n_cells, then a point of that cell: the offset (x + 2) * 2^-(level + 2) is exact
// (x + 2 = (v + 1) * 2^-51, v < 2^53), the cell's corner is exact, so each coordinate is ONE rounded addition.
template <bool kCells, class Grid>
__device__ __forceinline__ void next_sample(const Grid &g, Xorwow &rng, double &cr, double &ci) {
  if (kCells) {
    const uint32_t hi = xorwow_next(rng);
    const uint32_t lo = xorwow_next(rng);
    const unsigned long long ab = ((unsigned long long) hi << 32) | (unsigned long long) lo;
    const uint32_t j = (uint32_t) __umul64hi(ab, (unsigned long long) g.n_cells);  // < n_cells
    const uint32_t cell = g.cells[j];
    const uint32_t shift = (uint32_t) g.level + 2u;  // n = 4 * 2^level cells per side
    const uint32_t col = cell & ((1u << shift) - 1u);
    const uint32_t row = cell >> shift;
    const double x = sample_coordinate(rng);
    const double y = sample_coordinate(rng);
    const double lo_re = -2.0 + (double) col * g.cell_side;
    const double lo_im = -2.0 + (double) row * g.cell_side;
    const double off_re = (x + 2.0) * g.cell_scale;
    const double off_im = (y + 2.0) * g.cell_scale;
    cr = lo_re + off_re;
    ci = lo_im + off_im;
  } else {
    uniform_sample(rng, cr, ci);
  }
}

// The probe's sink: the bit of the cell that holds c.  (c + 2) * 2^level is exact; c = 2 exactly, which
// sample_coordinate can return, is clamped into the last cell.
template <class Grid>
__device__ __forceinline__ void mark_cell(const Grid &g, double cr, double ci) {
  const int n = 4 << g.level;
  int col = (int) ((cr + 2.0) * g.cells_per_unit);
  int row = (int) ((ci + 2.0) * g.cells_per_unit);
  col = col < 0 ? 0 : (col > n - 1 ? n - 1 : col);
  row = row < 0 ? 0 : (row > n - 1 ? n - 1 : row);
  const uint32_t index = (uint32_t) row * (uint32_t) n + (uint32_t) col;
  __hip_atomic_fetch_or(g.mask + (index >> 5), 1u << (index & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

}  // namespace cb
