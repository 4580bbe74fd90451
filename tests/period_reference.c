/* period_reference.c -- CPU restatement of the period-palette render (include/cudabrot_amd.h, "Period-palette render"),
 * for the tests only.  Plain C on the oracle's generator (oracle/liboracle.so), written from the definition; the steps, the
 * projection, the binning and the schedule's helpers are tests/bounded_reference.c's (and through it
 * tests/plot_reference.c's), included here.  Compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 * Two modes that must agree bit for bit on the three planes and on every counter but skipped_steps:
 *   mode 0  the definition: iterate to M; a bounded sample continues up to J = n_entries - 1 steps past z_M, without an
 *           escape test, for its period -- the least j with fma(dr, dr, di * di) <= eps, dr and di the parts of z_{M+j} - z_M,
 *           0 if there is none --, then plots (z_k, c) for k = 1 .. M, each adding the three weights of lut[period];
 *   mode 1  the product kernel's schedule (draw_periods_kernel): cycle compression at chunk boundaries of 60 steps with the
 *           refined Brent saves; the search walks from the point held -- z_s if an exact cycle z_k == z_s was found, else
 *           z_M -- rem = (M - s) mod p steps to the probe and then up to J steps; a zero entry is not replayed, its replay
 *           booked into skipped_steps; else the transient with weight 1 and ONE period with the weights of the bounded
 *           render, each multiplied by the entry's three.
 * Both note, per run, the class of every bounded sample under the kernel's schedule (period_extra), so that a test can
 * show that its inputs reach the paths they are meant to reach, and the steps the search makes. */
#include "bounded_reference.c"

/* Bounded samples by class: cycle_period (a) an exact cycle found by the schedule, period in 1 .. J; cycle_none (b) an
 * exact cycle found, period 0; tol_period (c) no exact cycle by M, period in 1 .. J; tol_none (d) no exact cycle, period
 * 0; rem_zero (e) an exact cycle with rem == 0, where the probe is z_s itself; zero_entry (f) an entry without weights,
 * which the product kernel does not replay.  search_steps: the steps of the search as the mode makes them (mode 1: the
 * rem steps to the probe included).  escaped: the samples that escape. */
typedef struct {
  uint64_t cycle_period, cycle_none, tol_period, tol_none, rem_zero, zero_entry, search_steps, escaped;
} period_extra;

static int period_returned(double r, double i, double pr, double pi, double eps) {
  const double dr = r - pr;
  const double di = i - pi;
  return fma(dr, dr, di * di) <= eps; /* a NaN compares false */
}

/* One sample (sr, si): z_0, and c as well unless c is fixed.  hist: three planes `plane` counters apart. */
static void period_sample(const orc_dims *d, uint64_t *hist, uint64_t plane, int max_iter, int formula, int degree,
                          int ship, const double *P, const double *c_fixed, const uint32_t *lut, int n_entries, double eps,
                          int mode, double sr, double si, int atomic, bounded_counters *cnt, period_extra *ex) {
  const int M = max_iter > 0 ? max_iter : 0;
  const int J = n_entries - 1;
  const double cr = c_fixed ? c_fixed[0] : sr, ci = c_fixed ? c_fixed[1] : si;
  double r = sr, i = si, saved_r = 0.0, saved_i = 0.0;
  int saved = 0, n = 0, s = M + 1, p = 0;
  cnt->samples++;
  for (int k = 1; k <= M; ++k) {
    if (plot_step(formula, degree, ship, cr, ci, &r, &i) > 4.0) { /* z_k escapes: nothing is added */
      cnt->too_fast++;
      cnt->iterate_steps += (uint64_t) k;
      ex->escaped++;
      return;
    }
    n = k;
    if (p == 0 && k % CHUNK == 0) { /* the kernel's schedule; the definition iterates on */
      if (saved > 0 && same_bits(r, saved_r) && same_bits(i, saved_i)) {
        s = saved;
        p = k - saved;
        if (mode == 1) break;
      } else if (bounded_brent_save((uint32_t) (k / CHUNK))) {
        saved_r = r;
        saved_i = i;
        saved = k;
      }
    }
  }
  cnt->never_escaped++;
  cnt->recorded++;
  cnt->iterate_steps += (uint64_t) M;
  cnt->replay_steps += (uint64_t) M;
  const int rem = p > 0 ? (M - s) % p : 0;
  /* the period */
  int period = 0;
  {
    /* mode 0: (r, i) is z_M.  mode 1: (r, i) is z_M, or z_k == z_s bit for bit, rem steps before the cycle point z_M is */
    if (mode == 1) {
      for (int j = 0; j < rem; ++j) {
        (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
        ex->search_steps++;
      }
    }
    const double probe_r = r, probe_i = i;
    for (int j = 1; j <= J; ++j) {
      (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
      ex->search_steps++;
      if (period_returned(r, i, probe_r, probe_i, eps)) {
        period = j;
        break;
      }
    }
  }
  if (p > 0) {
    if (period > 0) ex->cycle_period++; else ex->cycle_none++;
    ex->rem_zero += rem == 0;
  } else {
    if (period > 0) ex->tol_period++; else ex->tol_none++;
  }
  const uint32_t entry = lut[period] & 0xffffffu;
  const int end = (mode == 1 && p > 0) ? s - 1 + p : M;
  if (mode == 1) cnt->skipped_steps += (uint64_t) (M - n) + (uint64_t) (M - end);
  if (entry == 0u) {
    ex->zero_entry++;
    if (mode == 1) {
      cnt->skipped_steps += (uint64_t) end;
      return;
    }
  }
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  r = sr;
  i = si;
  for (int j = 1; j <= end; ++j) {
    (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
    const uint64_t w = (mode == 1 && j >= s) ? (uint64_t) ((M - j) / p) + 1u : 1u;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    for (int c = 0; c < 3; ++c) {
      const uint64_t weight = plot_weight(entry, c) * w;
      if (weight == 0u) continue;
      if (atomic) {
        __atomic_fetch_add(hist + (uint64_t) c * plane + index, weight, __ATOMIC_RELAXED);
      } else {
        hist[(uint64_t) c * plane + index] += weight;
      }
      cnt->increments += weight;
    }
  }
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample.  hist: three
 * planes of w*h counters; c_fixed NULL: c is the sample.  out and extra gain what these samples add. */
void period_draw(const orc_dims *d, uint64_t *hist, int max_iter, int formula, int degree, int ship, const double *P,
                 const double *c_fixed, const uint32_t *lut, int n_entries, double eps, int mode, orc_xorwow *states,
                 uint64_t n_threads, int samples_per_thread, bounded_counters *out, period_extra *extra, int n_omp) {
  bounded_counters total;
  period_extra total_ex;
  memset(&total, 0, sizeof(total));
  memset(&total_ex, 0, sizeof(total_ex));
  const uint64_t plane = (uint64_t) d->w * (uint64_t) d->h;
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    bounded_counters mine;
    period_extra mine_ex;
    memset(&mine, 0, sizeof(mine));
    memset(&mine_ex, 0, sizeof(mine_ex));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        period_sample(d, hist, plane, max_iter, formula, degree, ship, P, c_fixed, lut, n_entries, eps, mode, sr, si,
                      n_omp > 0, &mine, &mine_ex);
      }
    }
#pragma omp critical(period_counters_sum)
    {
      bounded_add((uint64_t *) &total, (const uint64_t *) &mine, sizeof(total) / sizeof(uint64_t));
      bounded_add((uint64_t *) &total_ex, (const uint64_t *) &mine_ex, sizeof(total_ex) / sizeof(uint64_t));
    }
  }
  bounded_add((uint64_t *) out, (const uint64_t *) &total, sizeof(total) / sizeof(uint64_t));
  bounded_add((uint64_t *) extra, (const uint64_t *) &total_ex, sizeof(total_ex) / sizeof(uint64_t));
}
