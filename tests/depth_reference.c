/* depth_reference.c -- CPU restatement of the depth render (include/cudabrot_amd.h, "Depth render"), for the tests only.
 * Written from the definition, not from the kernels; the step, the projection's operations, the binning of (u, v) and the
 * sample stream are plot_reference.c's, which is included, not restated.  Compiled by the tests like it:
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   depth_slice  the slice of one depth alone: s, or -1 for a depth outside the window
 *   depth_point  the depth of one point alone: d of (z, c) under D
 *   depth_draw   one launch: plot_draw without a table, every in-canvas point of an accepted orbit that is in depth adding
 *                1 to its pixel of plane s of N */
#include "plot_reference.c"

/* delta_d as the host makes it: (max - min) / (double) N, as cb_recompute_pixel_deltas makes delta_imag. */
static double depth_delta(double min, double max, int slices) { return (max - min) / (double) slices; }

/* The reference's binning of `im` with the window in the place of the canvas's rows. */
int depth_slice(double d, double min, double max, int slices) {
  if (d < min) return -1;
  const int s = (int) ((d - min) / depth_delta(min, max, slices));
  if (s < 0 || s >= slices) return -1;
  return s;
}

/* D is D[4]: columns (z_re, z_im, c_re, c_im). */
double depth_point(const double *D, double zr, double zi, double cr, double ci) {
  const double kd = fma(D[2], cr, D[3] * ci);
  return fma(D[0], zr, fma(D[1], zi, kd));
}

/* One sample (sr, si): z_0, and c as well unless c is fixed. */
static void depth_one_sample(const orc_dims *d, const orc_iters *it, int formula, int degree, int ship, int reject,
                             const double *P, const double *c_fixed, const double *D, double dmin, double dmax, int slices,
                             double sr, double si, uint64_t *hist, int atomic, plot_counters *cnt) {
  const int max = it->max_escape_iterations;
  const double cr = c_fixed ? c_fixed[0] : sr, ci = c_fixed ? c_fixed[1] : si;
  cnt->samples++;
  if (reject && (orc_in_main_cardioid(sr, si) || orc_in_order2_bulb(sr, si))) {
    cnt->rejected++;
    return;
  }
  /* escape index, and (plot_reference.c's note, not part of the definition) whether the orbit meets, at a multiple of
   * CHUNK steps below max, a point it was at an earlier multiple of CHUNK bit for bit */
  double r = sr, i = si;
  double br[MAX_BOUNDARIES], bi[MAX_BOUNDARIES];
  int boundaries = 0, repeated = 0;
  int k = 0;
  while (k < max && !(plot_step(formula, degree, ship, cr, ci, &r, &i) > 4.0)) {
    k++;
    if (k % CHUNK == 0 && k < max && !repeated) {
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
  const uint64_t plane_pixels = (uint64_t) d->w * (uint64_t) d->h;
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  const double kd = fma(D[2], cr, D[3] * ci);
  r = sr;
  i = si;
  for (int n = 0; n <= k; ++n) { /* replay z_1 .. z_{k+1} */
    (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
    cnt->replay_steps++;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    const double depth = fma(D[0], r, fma(D[1], i, kd));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    const int s = depth_slice(depth, dmin, dmax, slices);
    if (s < 0) continue;
    if (atomic) {
      __atomic_fetch_add(hist + (uint64_t) s * plane_pixels + index, 1u, __ATOMIC_RELAXED);
    } else {
      hist[(uint64_t) s * plane_pixels + index] += 1u;
    }
    cnt->increments++;
  }
}

/* plot_draw with a depth: hist is `slices` planes of w*h counters. */
void depth_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int formula, int degree, int ship, int reject,
                const double *P, const double *c_fixed, const double *D, double dmin, double dmax, int slices,
                orc_xorwow *states, uint64_t n_threads, int samples_per_thread, plot_counters *out, int n_omp) {
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
        depth_one_sample(d, it, formula, degree, ship, reject, P, c_fixed, D, dmin, dmax, slices, sr, si, hist, n_omp > 0,
                         &mine);
      }
    }
#pragma omp critical(depth_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
