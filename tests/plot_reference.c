/* plot_reference.c -- CPU restatement of the plotted renders (include/cudabrot_amd.h, "Projected render", "Multibrot
 * step", "Julia render", "Palette render", "Formula step", "Depth render", "Depth-palette render"), for the tests only.
 * Plain C on the oracle's generator and shortcuts (oracle/liboracle.so), written from the definitions, not from the
 * kernels; compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   plot_step         one step of one point
 *   plot_point        the plot of one point alone: (u, v) of (z, c) under P
 *   plot_depth        the depth of one point alone: d of (z, c) under D
 *   plot_slice        the slice of one depth alone: s, or -1 for a depth outside the window
 *   plot_weight       weight_j of an entry
 *   plot_slice_entry  the entry of one depth alone, or -1 for a depth outside the window
 *   plot_draw         one launch: samples_per_thread samples from each generator; c is the sample (c_fixed NULL) or fixed
 *                     (a Julia render: the sample is then z_0); a launch is a step, a source of c and a sink -- where an
 *                     in-canvas point of an accepted orbit goes, and with what weight:
 *                       no depth, no table  1 to its pixel of the one plane
 *                       table               the three weights of lut[k], k the escape index, to its pixel of three planes
 *                       depth               1 to its pixel of plane s of N, s the slice of its depth; none outside the window
 *                       depth and table     the three weights of lut[s] to its pixel of three planes; lut has N entries
 * plot_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments); without -fopenmp the pragmas are
 * ignored and it runs on one thread. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

#define CHUNK 60           /* steps between the points the product kernel compares */
#define MAX_BOUNDARIES 512 /* chunk boundaries remembered per sample: max_iter up to 30720 */

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
  /* not counters of the definition: the replay steps of the accepted orbits whose entry has no weight (what the product
   * kernel adds to skipped_steps on their account), and the samples whose orbit, at a multiple of CHUNK steps below max,
   * is bit for bit at a point it was at an earlier multiple of CHUNK (what the product kernel's early-out can retire) */
  uint64_t zero_entry_steps, chunk_repeats;
} plot_counters;

/* One step z <- step(c, z); returns |z'|^2 as tested.  formula 1 .. 5: the table of "Formula step" -- what is added to cr,
 * and the cross term's two factors (ni = fma(a, b, ci)).  formula 0, degree 2: the reference's step, ship != 0 its Burning
 * Ship variant, in the same three terms.  formula 0, degree 3 .. 8: degree - 1 multiplications by z, left to right, then
 * + c. */
double plot_step(int formula, int degree, int ship, double cr, double ci, double *r, double *i) {
  const double zr = *r, zi = *i;
  double nr, ni;
  if (formula == 0 && degree != 2) {
    double wr = zr, wi = zi;
    for (int n = 1; n < degree; ++n) {
      const double t = wi * zi;
      const double s = wi * zr;
      const double pr = fma(wr, zr, -t);
      const double pi = fma(wr, zi, s);
      wr = pr;
      wi = pi;
    }
    nr = cr + wr;
    ni = ci + wi;
  } else {
    const double ii = zi * zi;
    const double t = fma(zr, zr, -ii);
    double real_part, a, b;
    switch (formula) {
      case 1: real_part = t;       a = -(zr + zr);             b = zi;       break; /* tricorn */
      case 2: real_part = fabs(t); a = zr + zr;                b = zi;       break; /* celtic */
      case 3: real_part = fabs(t); a = fabs(zr) + fabs(zr);    b = fabs(zi); break; /* buffalo */
      case 4: real_part = t;       a = -(fabs(zr) + fabs(zr)); b = zi;       break; /* perpendicular */
      case 5: real_part = fabs(t); a = -(zr + zr);             b = zi;       break; /* celtic-tricorn */
      default:
        real_part = t;
        a = ship ? fabs(zr) + fabs(zr) : zr + zr;
        b = ship ? fabs(zi) : zi;
        break;
    }
    nr = cr + real_part;
    ni = fma(a, b, ci);
  }
  *r = nr;
  *i = ni;
  return fma(ni, ni, nr * nr);
}

/* P is P[2][4] row-major: rows (u, v), columns (z_re, z_im, c_re, c_im). */
void plot_point(const double *P, double zr, double zi, double cr, double ci, double *u, double *v) {
  const double ku = fma(P[2], cr, P[3] * ci);
  const double kv = fma(P[6], cr, P[7] * ci);
  *u = fma(P[0], zr, fma(P[1], zi, ku));
  *v = fma(P[4], zr, fma(P[5], zi, kv));
}

/* The binning of (u, v): the reference's IncrementPixelCounter with u for re and v for im. */
static int bin_of(const orc_dims *d, double u, double v, uint64_t *index) {
  if (u < d->min_real || v < d->min_imag) return 0;
  const int col = (int) ((u - d->min_real) / d->delta_real);
  const int row = (int) ((v - d->min_imag) / d->delta_imag);
  if (col < 0 || col >= d->w || row < 0 || row >= d->h) return 0;
  *index = (uint64_t) row * (uint64_t) d->w + (uint64_t) col;
  return 1;
}

/* D is D[4]: columns (z_re, z_im, c_re, c_im). */
double plot_depth(const double *D, double zr, double zi, double cr, double ci) {
  const double kd = fma(D[2], cr, D[3] * ci);
  return fma(D[0], zr, fma(D[1], zi, kd));
}

/* delta_d as the host makes it: (max - min) / (double) N, as cb_recompute_pixel_deltas makes delta_imag. */
static double depth_delta(double min, double max, int slices) { return (max - min) / (double) slices; }

/* The reference's binning of `im` with the window in the place of the canvas's rows. */
int plot_slice(double d, double min, double max, int slices) {
  if (d < min) return -1;
  const int s = (int) ((d - min) / depth_delta(min, max, slices));
  if (s < 0 || s >= slices) return -1;
  return s;
}

/* weight_j of an entry: plane 0 = R (bits 0-7), 1 = G (8-15), 2 = B (16-23); bits 24-31 are not read. */
uint64_t plot_weight(uint32_t entry, int plane) { return (uint64_t) ((entry >> (8 * plane)) & 0xffu); }

/* The entry of a depth: lut[s] without its unread bits for a depth in slice s of the window, -1 for a depth outside it. */
int64_t plot_slice_entry(double depth, double dmin, double dmax, int slices, const uint32_t *lut) {
  const int s = plot_slice(depth, dmin, dmax, slices);
  return s < 0 ? -1 : (int64_t) (lut[s] & 0xffffffu);
}

static int same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

/* One sample (sr, si): z_0, and c as well unless c is fixed.  D NULL: no depth. */
static void one_sample(const orc_dims *d, const orc_iters *it, int formula, int degree, int ship, int reject,
                       const double *P, const double *c_fixed, const uint32_t *lut, const double *D, double dmin,
                       double dmax, int slices, double sr, double si, uint64_t *hist, int atomic, plot_counters *cnt) {
  const int max = it->max_escape_iterations;
  const double cr = c_fixed ? c_fixed[0] : sr, ci = c_fixed ? c_fixed[1] : si;
  cnt->samples++;
  if (reject && (orc_in_main_cardioid(sr, si) || orc_in_order2_bulb(sr, si))) {
    cnt->rejected++;
    return;
  }
  /* escape index: the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max; z_0 is not tested */
  double r = sr, i = si;
  double br[MAX_BOUNDARIES], bi[MAX_BOUNDARIES];
  int boundaries = 0, repeated = 0;
  int k = 0;
  while (k < max && !(plot_step(formula, degree, ship, cr, ci, &r, &i) > 4.0)) {
    k++;
    if (k % CHUNK == 0 && k < max && !repeated) { /* z_k, tested and not escaping */
      for (int b = 0; b < boundaries && !repeated; ++b) repeated = same_bits(r, br[b]) && same_bits(i, bi[b]);
      if (boundaries < MAX_BOUNDARIES) {
        br[boundaries] = r;
        bi[boundaries] = i;
        boundaries++;
      }
    }
  }
  if (repeated) cnt->chunk_repeats++;
  if (k >= max) {
    cnt->never_escaped++;
    if (max > 0) cnt->iterate_steps += (uint64_t) max;
    return;
  }
  cnt->iterate_steps += (uint64_t) k + 1u;
  if (k < it->min_escape_iterations) {
    cnt->too_fast++;
    return;
  }
  cnt->recorded++;
  /* the orbit's entry: lut[k] of a table by escape index, else weight 1 in one plane -- under a depth the point's
   * slice says which plane, or (a table by depth) replaces the entry; no orbit is skipped on account of a colour then */
  const uint32_t orbit_entry = (lut && !D) ? lut[k] : 1u;
  if ((orbit_entry & 0xffffffu) == 0u) cnt->zero_entry_steps += (uint64_t) k + 1u;
  const uint64_t plane_pixels = (uint64_t) d->w * (uint64_t) d->h;
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  /* replay z_1 .. z_{k+1} */
  r = sr;
  i = si;
  for (int n = 0; n <= k; ++n) {
    (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
    cnt->replay_steps++;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    uint32_t entry = orbit_entry;
    uint64_t first_plane = 0u;
    if (D) {
      const double depth = plot_depth(D, r, i, cr, ci);
      const int64_t in_depth = lut ? plot_slice_entry(depth, dmin, dmax, slices, lut) : plot_slice(depth, dmin, dmax, slices);
      if (in_depth < 0) continue;
      if (lut) {
        entry = (uint32_t) in_depth;
      } else {
        first_plane = (uint64_t) in_depth;
      }
    }
    for (int j = 0; j < 3; ++j) {
      const uint64_t weight = plot_weight(entry, j);
      if (weight == 0u) continue;
      uint64_t *at = hist + (first_plane + (uint64_t) j) * plane_pixels + index;
      if (atomic) {
        __atomic_fetch_add(at, weight, __ATOMIC_RELAXED);
      } else {
        *at += weight;
      }
      cnt->increments += weight;
    }
  }
}

static void counters_add(plot_counters *dst, const plot_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(plot_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample.  hist: planes
 * of w*h counters -- one (lut NULL, D NULL), `slices` (D alone) or three (lut); lut: max_escape_iterations entries, or
 * `slices` with D; c_fixed NULL: c is the sample; reject: samples in the main cardioid or the period-2 bulb are counted
 * and dropped unseen (the caller's choice -- the product does so exactly for a sampled c under the reference's own
 * step). */
void plot_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int formula, int degree, int ship, int reject,
               const double *P, const double *c_fixed, const uint32_t *lut, const double *D, double dmin, double dmax,
               int slices, orc_xorwow *states, uint64_t n_threads, int samples_per_thread, plot_counters *out, int n_omp) {
  plot_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    plot_counters mine;
    memset(&mine, 0, sizeof(mine));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int s = 0; s < samples_per_thread; ++s) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_sample(d, it, formula, degree, ship, reject, P, c_fixed, lut, D, dmin, dmax, slices, sr, si, hist, n_omp > 0,
                   &mine);
      }
    }
#pragma omp critical(plot_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
