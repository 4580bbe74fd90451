/* bounded_reference.c -- CPU restatement of the bounded render (include/cudabrot_amd.h, "Bounded render"), for the tests
 * only.  Plain C on the oracle's generator (oracle/liboracle.so), written from the definition; the steps, the projection
 * and the binning are tests/plot_reference.c's, included here.  Compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 * Two modes that must agree bit for bit:
 *   mode 0  the definition: iterate to M, and if no z_k escaped, plot (z_k, c) for k = 1 .. M, each with weight 1;
 *   mode 1  cycle compression at chunk boundaries of 60 steps with the refined Brent save schedule (as
 *           draw_bounded_kernel): the transient z_1 .. z_{s-1} with weight 1, then ONE period in which z_{s+j} carries the
 *           weight floor((M - s - j) / p) + 1.
 * Both note, per run, what the kernel's schedule meets (bounded_extra), so that a test can show that its inputs reach the
 * branch they are meant to reach.  Each with an OpenMP variant (n_omp > 0: that many workers, atomic increments). */
#include "plot_reference.c"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments, skipped_steps;
} bounded_counters;

/* escaped: samples that escape; cycles: bounded samples whose z_k, at a multiple k <= M of 60 steps, is bit for bit the
 * point saved by the schedule; no_cycle: the other bounded samples; both_weights: cycles in which both weights q + 1 and q
 * occur ((M - s) % p < p - 1); at_m: cycles found at k == M; rem_zero: cycles with (M - s) % p == 0; in_canvas, off_canvas:
 * the M points of every bounded sample, by whether they are binned. */
typedef struct {
  uint64_t escaped, cycles, no_cycle, both_weights, at_m, rem_zero, in_canvas, off_canvas;
} bounded_extra;

static int bounded_brent_save(uint32_t chunks) {
  const int top = 31 - __builtin_clz(chunks);
  return top < 1 || (chunks & ((1u << (top - 1)) - 1u)) == 0u;
}

/* One sample (sr, si): z_0, and c as well unless c is fixed. */
static void bounded_sample(const orc_dims *d, uint64_t *hist, int max_iter, int formula, int degree, int ship,
                           const double *P, const double *c_fixed, int mode, double sr, double si, int atomic,
                           bounded_counters *cnt, bounded_extra *ex) {
  const int M = max_iter > 0 ? max_iter : 0;
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
  if (p > 0) {
    ex->cycles++;
    ex->both_weights += (M - s) % p < p - 1;
    ex->at_m += s + p == M;
    ex->rem_zero += (M - s) % p == 0;
  } else {
    ex->no_cycle++;
  }
  const int end = (mode == 1 && p > 0) ? s - 1 + p : M;
  if (mode == 1) cnt->skipped_steps += (uint64_t) (M - n) + (uint64_t) (M - end);
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
    if (!bin_of(d, u, v, &index)) {
      ex->off_canvas += w;
      continue;
    }
    ex->in_canvas += w;
    if (atomic) {
      __atomic_fetch_add(hist + index, w, __ATOMIC_RELAXED);
    } else {
      hist[index] += w;
    }
    cnt->increments += w;
  }
}

static void bounded_add(uint64_t *dst, const uint64_t *src, size_t words) {
  for (size_t k = 0; k < words; ++k) dst[k] += src[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample.  hist: one plane
 * of w*h counters; c_fixed NULL: c is the sample.  out and extra gain what these samples add. */
void bounded_draw(const orc_dims *d, uint64_t *hist, int max_iter, int formula, int degree, int ship, const double *P,
                  const double *c_fixed, int mode, orc_xorwow *states, uint64_t n_threads, int samples_per_thread,
                  bounded_counters *out, bounded_extra *extra, int n_omp) {
  bounded_counters total;
  bounded_extra total_ex;
  memset(&total, 0, sizeof(total));
  memset(&total_ex, 0, sizeof(total_ex));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    bounded_counters mine;
    bounded_extra mine_ex;
    memset(&mine, 0, sizeof(mine));
    memset(&mine_ex, 0, sizeof(mine_ex));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        bounded_sample(d, hist, max_iter, formula, degree, ship, P, c_fixed, mode, sr, si, n_omp > 0, &mine, &mine_ex);
      }
    }
#pragma omp critical(bounded_counters_sum)
    {
      bounded_add((uint64_t *) &total, (const uint64_t *) &mine, sizeof(total) / sizeof(uint64_t));
      bounded_add((uint64_t *) &total_ex, (const uint64_t *) &mine_ex, sizeof(total_ex) / sizeof(uint64_t));
    }
  }
  bounded_add((uint64_t *) out, (const uint64_t *) &total, sizeof(total) / sizeof(uint64_t));
  bounded_add((uint64_t *) extra, (const uint64_t *) &total_ex, sizeof(total_ex) / sizeof(uint64_t));
}
