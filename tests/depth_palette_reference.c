/* depth_palette_reference.c -- CPU restatement of the depth-palette render (include/cudabrot_amd.h, "Depth-palette
 * render"), for the tests only.  Written from the definition, not from the kernels; the depth of a point, its slice and
 * the window's step are depth_reference.c's, and through it the step, the projection's operations, the binning of (u, v)
 * and the sample stream plot_reference.c's: both are included, not restated.  What stands here is the one thing the
 * definition changes -- where a point that is on the canvas and in depth goes, and with what weight.  Compiled by the
 * tests like them:
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   depth_palette_weight  weight_j of an entry
 *   depth_palette_entry   the entry of one depth alone, or -1 for a depth outside the window
 *   depth_palette_draw    one launch: depth_draw with a table of `slices` entries, every in-canvas point of an accepted
 *                         orbit that is in depth adding the three weights of lut[s] to its pixel of three planes */
#include "depth_reference.c"

/* weight_j of an entry: plane 0 = R (bits 0-7), 1 = G (8-15), 2 = B (16-23); bits 24-31 are not read. */
uint64_t depth_palette_weight(uint32_t entry, int plane) { return (uint64_t) ((entry >> (8 * plane)) & 0xffu); }

/* The entry of a depth: lut[s] without its unread bits for a depth in slice s of the window, -1 for a depth outside it. */
int64_t depth_palette_entry(double depth, double dmin, double dmax, int slices, const uint32_t *lut) {
  const int s = depth_slice(depth, dmin, dmax, slices);
  return s < 0 ? -1 : (int64_t) (lut[s] & 0xffffffu);
}

/* One sample (sr, si): z_0, and c as well unless c is fixed. */
static void depth_palette_one_sample(const orc_dims *d, const orc_iters *it, int formula, int degree, int ship, int reject,
                                     const double *P, const double *c_fixed, const double *D, double dmin, double dmax,
                                     int slices, const uint32_t *lut, double sr, double si, uint64_t *hist, int atomic,
                                     plot_counters *cnt) {
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
  r = sr;
  i = si;
  for (int n = 0; n <= k; ++n) { /* replay z_1 .. z_{k+1} */
    (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
    cnt->replay_steps++;
    double u, v;
    plot_point(P, r, i, cr, ci, &u, &v);
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    const int64_t entry = depth_palette_entry(depth_point(D, r, i, cr, ci), dmin, dmax, slices, lut);
    if (entry < 0) continue;
    for (int j = 0; j < 3; ++j) {
      const uint64_t weight = depth_palette_weight((uint32_t) entry, j);
      if (weight == 0u) continue;
      if (atomic) {
        __atomic_fetch_add(hist + (uint64_t) j * plane_pixels + index, weight, __ATOMIC_RELAXED);
      } else {
        hist[(uint64_t) j * plane_pixels + index] += weight;
      }
      cnt->increments += weight;
    }
  }
}

/* depth_draw with a table: hist is three planes of w*h counters, lut `slices` entries. */
void depth_palette_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int formula, int degree, int ship,
                        int reject, const double *P, const double *c_fixed, const double *D, double dmin, double dmax,
                        int slices, const uint32_t *lut, orc_xorwow *states, uint64_t n_threads, int samples_per_thread,
                        plot_counters *out, int n_omp) {
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
        depth_palette_one_sample(d, it, formula, degree, ship, reject, P, c_fixed, D, dmin, dmax, slices, lut, sr, si, hist,
                                 n_omp > 0, &mine);
      }
    }
#pragma omp critical(depth_palette_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
