// Host-side scalar solve of one sizing problem, shared by the torch
// binding (queue_solver.cpp: CPU at::parallel_for + HIP dispatch glue)
// and the torch-free pybind11/numpy binding (queue_solver_cpu.cpp) used
// in the slim controller image.  Semantics mirror
// core.create_allocation's non-zero-load body (see queue_solver.cpp's
// header comment for the reference citation); the solve itself is
// queue_core.h's solve_row, here over a table in host memory.
#pragma once

#include <cmath>
#include <vector>

#include "queue_core.h"

namespace wva {

// Table length the compact policy needs for a row: trunc(N), 0 if invalid.
inline int row_compact_length(const double *pr) {
  return row_valid(pr) ? (int)pr[P_MAX_BATCH] : 0;
}

// inclusive sum cum[n] = sum_{i<=n} log_mu(i) over the first `len` states
inline void fill_cum(const Parms &p, int len, double *cum) {
  double acc = 0.0;
  for (int n = 0; n < len; ++n) {
    acc += log_mu(p, n);
    cum[n] = acc;
  }
}

// lf[i] = ln i! for i in [0, len): the waiting-time tail's table.  It does
// not depend on the row, so a batch fills one, as long as its longest tail
// sum, and every row reads it.
inline std::vector<double> log_factorials(long long len) {
  std::vector<double> lf((size_t)(len > 0 ? len : 0));
  double acc = 0.0;
  for (long long i = 0; i < len; ++i) {
    if (i > 0) acc += log((double)i);
    lf[(size_t)i] = acc;
  }
  return lf;
}

// P(TTFT > target_ttft) at lam over either table policy below (queue_core.h,
// "Waiting-time tail"): the mean-model evaluation, then the windowed tail sum
// over lf.  cum_last = cum[N-1], which both tables hold.
template <typename Table>
inline double host_exceedance(const Table &table, const double *lf, double cum_last,
                              double lam, double target_ttft) {
  const Parms &p = table.p;
  const double logp_n = (double)p.max_batch * log(lam) - cum_last;
  const TailSweep w = tail_sweep_of(p, table.eval(lam), logp_n, lam, target_ttft);
  if (w.certain) return 1.0;
  return tail_probability(w, tail_sum(w, [lf](int i) { return lf[i]; }, 0, 1));
}

// Table policies of solve_one: how long a row's table is, how it is filled,
// and which eval_model* reads it.  Each is an evaluator for solve_row.  The
// constructor WRITES the caller's scratch table (the log_mu scan) and the
// object then only reads it.  lf is log_factorials over at least 10 * N
// entries for a row with ttft_tail > 0, and is not read otherwise.

// K = 11 * N doubles, evaluated inside the significance window (state_window)
struct HostFullTable {
  static constexpr bool kReadsLogFactorials = true;
  static int length(const double *pr) { return row_chain_length(pr); }
  const Parms &p;
  const double *cum;
  int K;
  const double *lf;
  HostFullTable(const Parms &parms, double *table, const double *log_fact = nullptr)
      : p(parms), cum(table), K(parms.max_batch * (1 + kMaxQueueToBatchRatio)), lf(log_fact) {
    fill_cum(p, K, table);
  }
  Stats eval(double lam) const { return eval_model(p, cum, K, lam); }
  double exceedance(double lam, double target_ttft) const {
    return host_exceedance(*this, lf, cum[p.max_batch - 1], lam, target_ttft);
  }
};

// N doubles (queue_core.h, "Compact table"); no window
struct HostCompactTable {
  static constexpr bool kReadsLogFactorials = true;
  static int length(const double *pr) { return row_compact_length(pr); }
  const Parms &p;
  const double *cum;
  double log_mu_n;
  const double *lf;
  HostCompactTable(const Parms &parms, double *table, const double *log_fact = nullptr)
      : p(parms), cum(table), log_mu_n(log_mu(parms, parms.max_batch - 1)), lf(log_fact) {
    fill_cum(p, p.max_batch, table);
  }
  Stats eval(double lam) const { return eval_model_compact(p, cum, log_mu_n, lam); }
  double exceedance(double lam, double target_ttft) const {
    return host_exceedance(*this, lf, cum[p.max_batch - 1], lam, target_ttft);
  }
};

// The compact table with the tail by the Poisson recurrence (queue_core.h,
// tail_sum_chunk): the window as one chunk, no log-factorial table (the third
// argument is accepted and ignored, and the bindings fill none).  The mean
// model is HostCompactTable's, bit for bit; it is the host reference of the
// compact tail kernel, not a routing target.
struct HostTailCompactTable : HostCompactTable {
  static constexpr bool kReadsLogFactorials = false;
  HostTailCompactTable(const Parms &parms, double *table, const double * = nullptr)
      : HostCompactTable(parms, table) {}
  double exceedance(double lam, double target_ttft) const {
    const double logp_n = (double)p.max_batch * log(lam) - cum[p.max_batch - 1];
    const TailSweep w = tail_sweep_of(p, eval(lam), logp_n, lam, target_ttft);
    if (w.certain) return 1.0;
    return tail_probability(w, tail_centre_term(w) * tail_sum_chunk(w, 0, 1));
  }
};

// HostTailCompactTable plus the occupancy tail (queue_core.h, "Occupancy
// tail"): the evaluator of solve_allocations_ptile, the host reference of the
// percentile kernel and the CPU route of rows that carry an itl_tail.  TTFT
// side, mean model and table are the parent's, bit for bit.
struct HostPtileTable : HostTailCompactTable {
  double itl_tail;
  HostPtileTable(const Parms &parms, double *table, double itl_eps)
      : HostTailCompactTable(parms, table), itl_tail(itl_eps) {}
  double itl_eps() const { return itl_tail; }
  double itl_exceedance(double lam, int c) const {
    const OccupancySweep w = occupancy_sweep_of(p, cum, log_mu_n, lam);
    double all, upper;
    occupancy_sums(w, cum, p.max_batch, log_mu_n, c, 0, 1, &all, &upper);
    return occupancy_tail(w, all, upper);
  }
};

// solve_one over HostPtileTable: itl_eps is the row's itl_tail (0: size to the
// mean ITL).  cum must hold row_compact_length(pr) doubles.
inline void solve_one_ptile(const double *pr, double *out, double *cum, double scv,
                            double tail_eps, double itl_eps) {
  for (int f = 0; f < RESULT_FIELDS; ++f) out[f] = 0.0;
  if (!row_valid(pr, scv, tail_eps, itl_eps)) return;
  const Parms p = parms_from_problem(pr, scv, tail_eps);
  const HostPtileTable table(p, cum, itl_eps);
  const RowValues vals = solve_row(pr, p, table);
  out[R_FEASIBLE] = vals.feasible;
  out[R_REPLICAS] = vals.replicas;
  out[R_RATE_STAR] = vals.rate_star;
  out[R_ITL] = vals.itl;
  out[R_TTFT] = vals.ttft;
  out[R_RHO] = vals.rho;
}

// Scalar solve of one problem (CPU path).  cum must hold Table::length(pr)
// doubles; a row that breaks the contract of queue_core.h yields the
// all-zero row and touches no table.  scv is the row's service-time cs^2
// (1.0: Markovian); it only enters through Parms::wait_scale in eval_ttft_of.
// tail_eps is the row's ttft_tail (0: size to the mean TTFT) and lf the
// batch's log_factorials, at least batch_tail_length long.
template <typename Table>
inline void solve_one(const double *pr, double *out, double *cum, double scv = 1.0,
                      double tail_eps = 0.0, const double *lf = nullptr) {
  for (int f = 0; f < RESULT_FIELDS; ++f) out[f] = 0.0;
  if (!row_valid(pr, scv, tail_eps)) return;
  const Parms p = parms_from_problem(pr, scv, tail_eps);
  const Table table(p, cum, lf);  // fills cum: the O(table length) build happens here
  const RowValues vals = solve_row(pr, p, table);
  out[R_FEASIBLE] = vals.feasible;
  out[R_REPLICAS] = vals.replicas;
  out[R_RATE_STAR] = vals.rate_star;
  out[R_ITL] = vals.itl;
  out[R_TTFT] = vals.ttft;
  out[R_RHO] = vals.rho;
}

// TTFT quantile of one row (queue_core.h, "TTFT quantile"), sequentially: the
// compact table, one mean evaluation at the row's rate, then binary_search
// over t on the tail sum.  cum must hold N doubles and lf 10 * N log-factorials
// (row_compact_length, quantile_tail_length); out gets (valid, q).
inline void quantile_one(const double *pr, double rate, double eps, double *out, double *cum,
                         const double *lf, double scv = 1.0) {
  out[Q_VALID] = out[Q_TTFT] = 0.0;
  if (!row_valid(pr, scv)) return;
  const Parms p = parms_from_problem(pr, scv);
  if (!quantile_inputs_valid(p, rate, eps)) return;
  const HostCompactTable table(p, cum);
  const double lam = rate / 1000.0;
  const double logp_n = (double)p.max_batch * log(lam) - cum[p.max_batch - 1];
  const QuantileRow q = quantile_row_of(p, table.eval(lam), logp_n, lam, eps);
  double t = 0.0;
  if (q.p_wait > eps) {
    auto y = [&](double at) {
      if (!(at > 0.0)) return q.p_wait;
      const TailSweep w = tail_sweep_at(q, at);
      return tail_probability(w, tail_sum(w, [lf](int i) { return lf[i]; }, 0, 1));
    };
    binary_search(0.0, q.t_hi, eps, y, &t);
  }
  out[Q_VALID] = 1.0;
  out[Q_TTFT] = quantile_ttft(p, q, t);
}

// quantile_one without the log-factorial table: y(t) by queue_core.h's
// quantile_sum_chunk, over the kQuantileChunks chunks a wave of the compact
// quantile kernel takes one per lane, summed here in sequence.  The host
// reference of that kernel, not a routing target; cum must hold N doubles.
inline void quantile_one_compact(const double *pr, double rate, double eps, double *out,
                                 double *cum, double scv = 1.0) {
  out[Q_VALID] = out[Q_TTFT] = 0.0;
  if (!row_valid(pr, scv)) return;
  const Parms p = parms_from_problem(pr, scv);
  if (!quantile_inputs_valid(p, rate, eps)) return;
  const HostCompactTable table(p, cum);
  const double lam = rate / 1000.0;
  const double logp_n = (double)p.max_batch * log(lam) - cum[p.max_batch - 1];
  const QuantileRow q = quantile_row_of(p, table.eval(lam), logp_n, lam, eps);
  double t = 0.0;
  if (q.p_wait > eps) {
    const double growth = quantile_growth(q);
    auto y = [&](double at) {
      if (!(at > 0.0)) return q.p_wait;
      const TailSweep w = tail_sweep_at(q, at);
      double sum = 0.0;
      for (int part = 0; part < kQuantileChunks; ++part) {
        sum += quantile_sum_chunk(w, growth, part, kQuantileChunks);
      }
      return tail_probability(w, tail_centre_term(w) * sum);
    };
    binary_search(0.0, q.t_hi, eps, y, &t);
  }
  out[Q_VALID] = 1.0;
  out[Q_TTFT] = quantile_ttft(p, q, t);
}

// ITL quantile of one row (queue_core.h, "ITL quantile"): the compact table,
// then itl_quantile_row's one sweep and scan at the row's rate.  cum and suffix
// must each hold N doubles (row_compact_length); out gets (valid, q).  No cs^2:
// occupancy does not depend on the wait scale.
inline void itl_quantile_one(const double *pr, double rate, double eps, double *out, double *cum,
                             double *suffix) {
  out[Q_VALID] = out[Q_ITL] = 0.0;
  if (!row_valid(pr)) return;
  const Parms p = parms_from_problem(pr);
  if (!quantile_inputs_valid(p, rate, eps)) return;
  const HostCompactTable table(p, cum);
  const int b = itl_quantile_row(p, cum, table.log_mu_n, rate / 1000.0, eps, suffix);
  out[Q_VALID] = 1.0;
  out[Q_ITL] = decode_time(p, (double)b);
}

// Length of the log-factorial table quantile_one needs for a batch: 10 * N of
// its largest valid row.
inline long long quantile_tail_length(const double *pr, long long rows) {
  long long longest = 0;
  for (long long i = 0; i < rows; ++i) {
    const long long len =
        (long long)row_compact_length(pr + i * PROBLEM_FIELDS) * kMaxQueueToBatchRatio;
    if (len > longest) longest = len;
  }
  return longest;
}

// Scratch one thread needs for any row of a batch: the longest table, >= 1.
template <typename Table>
inline int batch_table_length(const double *pr, long long rows) {
  int longest = 1;
  for (long long i = 0; i < rows; ++i) {
    const int len = Table::length(pr + i * PROBLEM_FIELDS);  // 0 if invalid
    if (len > longest) longest = len;
  }
  return longest;
}

// Length of the log-factorial table a batch needs: 10 * N of its largest
// valid row that carries a ttft_tail, 0 without a vector or for a policy that
// reads none.
template <typename Table>
inline long long batch_tail_length(const double *pr, const double *tail, long long rows) {
  long long longest = 0;
  if (tail == nullptr || !Table::kReadsLogFactorials) return longest;
  for (long long i = 0; i < rows; ++i) {
    const double *row = pr + i * PROBLEM_FIELDS;
    if (!(tail[i] > 0.0) || !row_valid(row)) continue;
    const long long len = (long long)row[P_MAX_BATCH] * kMaxQueueToBatchRatio;
    if (len > longest) longest = len;
  }
  return longest;
}

}  // namespace wva
