// color_math.h -- the arithmetic of the colour stage (include/cudabrot_amd.h, "Colour image"), ONE definition for
// the host restatement (color_host.cpp) and the composite kernel (color.hip), so that both evaluate the same IEEE
// operations in the same order.  Built with -ffp-contract=off everywhere: nothing here may be fused.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/cudabrot_amd.h"

#ifdef __HIP__  // compiled as HIP (color.hip); plain C++ on the host (color_host.cpp)
#include <hip/hip_runtime.h>
#define CB_COLOR_FN __host__ __device__ __forceinline__
#else
#define CB_COLOR_FN inline
#endif

namespace cb {

// The levels of one plane, and 1 / (white - black) as the host evaluates it (0 when white <= black: unused).
struct PlaneLevels {
  uint32_t black, white;
  double inv;
};

// Step 2: the stretched value s in [0, 1].
CB_COLOR_FN double color_stretch(uint32_t v, const PlaneLevels &l) {
  if (v <= l.black) return 0.0;
  if (v >= l.white) return 1.0;
  return (double) (v - l.black) * l.inv;
}

CB_COLOR_FN uint32_t color_unit_to_u16(double c) { return (uint32_t) floor(c * 65535.0 + 0.5); }

CB_COLOR_FN double color_hsl_channel(double p, double q, double t) {
  t = t - floor(t);
  if (t < 1.0 / 6.0) return p + ((q - p) * 6.0) * t;
  if (t < 0.5) return q;
  if (t < 2.0 / 3.0) return p + ((q - p) * 6.0) * (2.0 / 3.0 - t);
  return p;
}

CB_COLOR_FN double color_clamp01(double c) { return c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c); }

// Steps 3 and 4: the three stretched values -> R, G, B as u16 values (host order; the caller swaps for the file).
CB_COLOR_FN void color_compose(int compose, double hue_shift, double s0, double s1, double s2, uint32_t rgb[3]) {
  if (compose == CB_COMPOSE_RGB) {
    rgb[0] = color_unit_to_u16(s0);
    rgb[1] = color_unit_to_u16(s1);
    rgb[2] = color_unit_to_u16(s2);
    return;
  }
  double h = s0 + hue_shift;
  h = h - floor(h);
  const double S = s1, L = s2;
  const double q = L < 0.5 ? L * (1.0 + S) : (L + S) - L * S;
  const double p = 2.0 * L - q;
  rgb[0] = color_unit_to_u16(color_clamp01(color_hsl_channel(p, q, h + 1.0 / 3.0)));
  rgb[1] = color_unit_to_u16(color_clamp01(color_hsl_channel(p, q, h)));
  rgb[2] = color_unit_to_u16(color_clamp01(color_hsl_channel(p, q, h - 1.0 / 3.0)));
}

CB_COLOR_FN uint32_t color_swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }

// The key of the equalised image (include/cudabrot_amd.h, "Equalised image"), ONE definition as well, for
// cb_equalize_key (host_output.cpp) and the two kernels (equalize.hip): the 11 most significant bits of a counter and
// where they stand.  A count-leading-zeros, a shift and an add; below 2048 the shift is 0 and the key is the count.
CB_COLOR_FN uint32_t equalize_key(uint64_t c) {
  const uint32_t s = c < 2048u ? 0u : 53u - (uint32_t) __builtin_clzll(c);  // floor(log2 c) - 10
  return (s << 10) + (uint32_t) (c >> s);
}

// ---- host side of the levels (color_host.cpp) ----

// 1 if p is a valid cb_color_params (compose, percentages, hue shift), else 0.
int color_params_ok(const cb_color_params *p);
// The ranks of step 1 for n pixels: nb (black) and nw (white).
void color_ranks(uint64_t n, const cb_color_params *p, uint64_t *nb, uint64_t *nw);
// Over bins[0..n_bins): the smallest k with sum(bins[0..k]) > rank, and *below = sum(bins[0..k)).
uint32_t color_select_low(const uint64_t *bins, uint32_t n_bins, uint64_t rank, uint64_t *below);
// Over bins[0..n_bins): the largest k with sum(bins[k..n_bins)) > rank, and *above = sum(bins(k..n_bins)).
uint32_t color_select_high(const uint64_t *bins, uint32_t n_bins, uint64_t rank, uint64_t *above);
// black, white -> PlaneLevels (inv evaluated here, on the host).
PlaneLevels color_plane_levels(uint32_t black, uint32_t white);

}  // namespace cb
