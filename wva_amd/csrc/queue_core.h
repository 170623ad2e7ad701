// Shared scalar math for the batched state-dependent M/M/1/K allocation
// sizing kernel.  Mirrors wva_amd/analyzer (which itself re-implements the
// behavior of /root/reference/pkg/analyzer) in double precision:
//   - service rates  mu(b) = b / (prefill(b) + numDecode * decode(b))
//   - product-form state probabilities in log space (softmax-normalized)
//   - monotone bisection with boundary-region classification
//   - Size(): max rate meeting TTFT/ITL targets; TPS as lambdaMax*0.9
//
// Used by both the CPU (OpenMP) path and the gfx950 HIP kernel.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define WVA_HD __host__ __device__ inline
#else
#define WVA_HD inline
#endif

namespace wva {

constexpr double kEpsilon = 0.001;           // rate-range disturbance
constexpr double kStabilityFraction = 0.1;   // TPS backoff fraction
constexpr double kTolerance = 1e-6;          // bisection relative tolerance
constexpr int kMaxIterations = 100;          // bisection iteration cap
constexpr int kMaxQueueToBatchRatio = 10;    // K = (1 + ratio) * N

// Problem layout: one row of 12 doubles.
//
// Row contract (row_valid below; every solver — this header's host and
// device users and ops/batched.py's Python path — enforces the same one).
// A row is valid iff
//   - every field is finite;
//   - alpha, beta, gamma, delta >= 0;
//   - trunc(N) >= 1 and the chain length 11 * N fits an int;
//   - trunc(out_tokens) >= 1 (and fits an int);
//   - in_tokens >= 0;
//   - every target >= 0.
// An invalid row yields the all-zero result row, as the analyzer's check()
// methods reject it.  in_tokens, out_tokens, N and min_replicas are
// truncated toward zero (Python's int()), so a replica count is always
// integral.
//
// M/G/1 correction (per-row service-time cs^2):
//   - a sizing row may carry a service-time cs^2, scv;
//   - wait_scale = (1 + scv) / 2;
//   - TTFT is wait * wait_scale + prefill(eff_conc) wherever it is
//     evaluated: in the bisection and in the final R_TTFT;
//   - nothing else changes; the wait >= 0 clamp stays before the scaling;
//   - scv must be finite and >= 0; any other value gives the all-zero
//     result row in every implementation (QueueAnalyzer rejects scv < 0,
//     the native guard also rejects NaN and inf);
//   - the -1 sentinel means "use the fleet value"; it is resolved on the
//     host, and a kernel never sees it;
//   - the 12-column problem layout and the 6-column result layout do not
//     change: scv travels as a separate optional float64 vector of length B
//     (absent means 1.0 for every row, the Markovian model).
// No vector, or a vector of all 1.0, gives results bit-identical to the
// Markovian ones (x * 1.0 is exact, and fma(x, 1.0, y) rounds x + y).
//
// TTFT percentile (per-row waiting-time tail, "Waiting-time tail" below):
//   - a sizing row may carry ttft_tail = eps, the allowed probability that
//     TTFT exceeds target_ttft (p95 is eps = 0.05);
//   - eps = 0 means "mean TTFT": the search compares the mean TTFT with the
//     target, as it always did;
//   - for eps > 0 the TTFT search runs on y(lam) = P(W > t(lam)) against the
//     target value eps, with t(lam) = (target_ttft - prefill(eff_conc(lam)))
//     / wait_scale and y = 1 when t <= 0 (the M/G/1 scaling stretches the
//     waiting time by wait_scale, as it scales the mean); binary_search and
//     classify_bracket are the same: eps below y(lam_min) is infeasible, eps
//     above y(lam_max) gives lam_max;
//   - the ITL search, the TPS back-off, the replica count and the final
//     evaluation do not change, and R_TTFT stays the predicted MEAN TTFT at
//     the final rate: only lam* moves, and through it the replica count;
//   - eps must be finite with 0 <= eps < 1; any other value (NaN, +-inf,
//     negative, >= 1) gives the all-zero result row in every implementation;
//   - a row with target_ttft = 0 ignores a valid eps;
//   - the layouts do not change: eps travels as a separate optional float64
//     vector of length B, like scv (absent means 0 for every row).
// No vector, or a vector of all 0, gives results bit-identical to the ones
// without it on every path.
// The tail sum has two evaluations of the same model and window: tail_sum
// over a log-factorial table (the tail kernel, N <= ~700, and the host
// solvers), and tail_sum_chunk, the Poisson recurrence without a table (the
// compact tail kernel, N <= ~7800, and its host reference
// solve_allocations_tail_compact).  They differ by rounding only.
//
// ITL percentile (per-row occupancy tail, "Occupancy tail" below):
//   - a sizing row may carry itl_tail = eps, the allowed fraction of tokens
//     whose ITL exceeds target_itl (p95 is eps = 0.05);
//   - eps = 0 means "mean ITL": the search compares decode_time at the mean
//     effective concurrency with the target, as it always did;
//   - for eps > 0 the ITL search runs on y(lam), the token-weighted share of
//     decode steps slower than target_itl, against the target value eps;
//     binary_search and classify_bracket are the same: no batch size meeting
//     the target (c = 0, y = 1) is infeasible, every batch size meeting it
//     (c = N, y = 0) gives lam_max;
//   - the TTFT search (mean or ttft_tail), the TPS back-off, the replica count
//     and the final evaluation do not change, and R_ITL stays the predicted
//     MEAN ITL at the final rate;
//   - eps must be finite with 0 <= eps < 1; any other value gives the all-zero
//     result row in every implementation;
//   - a row with target_itl = 0 ignores a valid eps;
//   - the layouts do not change: eps travels as a separate optional float64
//     vector of length B (absent means 0 for every row), and composes with scv
//     and ttft_tail on the same row.
// No vector, or a vector of all 0, gives results bit-identical to the ones
// without it on every path.
enum ProblemField {
  P_ALPHA = 0,    // decode base (ms), >= 0
  P_BETA,         // decode slope (ms per batch unit), >= 0
  P_GAMMA,        // prefill base (ms), >= 0
  P_DELTA,        // prefill slope (ms per token per batch unit), >= 0
  P_IN_TOKENS,    // average input tokens, >= 0, truncated
  P_OUT_TOKENS,   // average output tokens, truncated >= 1
  P_MAX_BATCH,    // N, truncated >= 1
  P_TARGET_TTFT,  // ms; 0 disables, < 0 invalid
  P_TARGET_ITL,   // ms; 0 disables, < 0 invalid
  P_TARGET_TPS,   // tokens/s; 0 disables, < 0 invalid
  P_TOTAL_RATE,   // req/s (> 0; zero-load handled by the host)
  P_MIN_REPLICAS, // minimum replica count, truncated
  PROBLEM_FIELDS
};

// Result layout: one row of 6 doubles.
enum ResultField {
  R_FEASIBLE = 0, // 1.0 feasible / 0.0 infeasible
  R_REPLICAS,     // number of replicas
  R_RATE_STAR,    // max per-replica rate meeting targets (req/s)
  R_ITL,          // predicted decode time per token at the final rate (ms)
  R_TTFT,         // predicted wait + prefill at the final rate (ms)
  R_RHO,          // avg-in-service / max-batch, clamped to [0,1]
  RESULT_FIELDS
};

struct Parms {
  double alpha, beta, gamma, delta;
  double in_tokens;
  int out_tokens;
  int max_batch;   // N
  int num_decode;  // out_tokens-1, or 1 for decode-only single-token
  double wait_scale;  // (1 + scv) / 2; 1.0 is the Markovian model
  double tail_eps;    // allowed P(TTFT > target); 0 sizes to the mean TTFT
};

// largest N whose chain length (1 + ratio) * N still fits an int
constexpr int kMaxBatchLimit = 2147483647 / (1 + kMaxQueueToBatchRatio);

// The row contract above.  Ordered compares are false for NaN, so each
// test is written to hold only for a proper value.  Branch-free (& rather
// than && or early returns): the kernels run this before anything else,
// and nothing in it should make one load wait for another's compare.
// scv is the row's service-time cs^2 (1.0 when the launch carries none):
// finite and >= 0, so the -1 sentinel never passes.  tail_eps is the row's
// ttft_tail (0 when the launch carries none): 0 <= eps < 1.  itl_eps is the
// row's itl_tail under the same rule.  A target_itl that equals some
// decode_time(m) to the last bit is outside the contract: the threshold count
// below may then differ by one between two compilers' roundings of alpha +
// beta * m.
WVA_HD bool row_valid(const double *pr, double scv = 1.0, double tail_eps = 0.0,
                      double itl_eps = 0.0) {
  bool ok = (scv >= 0.0) & (scv <= 1.7976931348623157e308);
  ok &= (tail_eps >= 0.0) & (tail_eps < 1.0);
  ok &= (itl_eps >= 0.0) & (itl_eps < 1.0);
  for (int f = 0; f < PROBLEM_FIELDS; ++f) {
    ok &= fabs(pr[f]) <= 1.7976931348623157e308;  // fails NaN, +-inf
  }
  ok &= (pr[P_ALPHA] >= 0.0) & (pr[P_BETA] >= 0.0) & (pr[P_GAMMA] >= 0.0) &
        (pr[P_DELTA] >= 0.0);
  ok &= (pr[P_MAX_BATCH] >= 1.0) & (pr[P_MAX_BATCH] < (double)kMaxBatchLimit + 1.0);
  ok &= (pr[P_OUT_TOKENS] >= 1.0) & (pr[P_OUT_TOKENS] < 2147483648.0);
  ok &= pr[P_IN_TOKENS] >= 0.0;
  ok &= (pr[P_TARGET_TTFT] >= 0.0) & (pr[P_TARGET_ITL] >= 0.0) & (pr[P_TARGET_TPS] >= 0.0);
  return ok;
}

// Model constants of a VALID row (the int casts are undefined otherwise).
WVA_HD Parms parms_from_problem(const double *pr, double scv = 1.0, double tail_eps = 0.0) {
  Parms p;
  p.alpha = pr[P_ALPHA];
  p.beta = pr[P_BETA];
  p.gamma = pr[P_GAMMA];
  p.delta = pr[P_DELTA];
  p.in_tokens = trunc(pr[P_IN_TOKENS]);
  p.out_tokens = (int)pr[P_OUT_TOKENS];
  p.max_batch = (int)pr[P_MAX_BATCH];
  p.num_decode = p.out_tokens - 1;
  if (p.in_tokens == 0.0 && p.out_tokens == 1) p.num_decode = 1;
  p.wait_scale = (1.0 + scv) / 2.0;
  p.tail_eps = tail_eps;
  return p;
}

// Chain length K = 11 * N of a row; 0 for an invalid row, which needs no
// table at all.  It sizes tables from the 12 columns alone: a row rejected
// for its scv only reserves a table nobody fills.
WVA_HD int row_chain_length(const double *pr) {
  return row_valid(pr) ? (int)pr[P_MAX_BATCH] * (1 + kMaxQueueToBatchRatio) : 0;
}

WVA_HD double prefill_time(const Parms &p, double batch) {
  return p.in_tokens == 0.0 ? 0.0 : p.gamma + p.delta * p.in_tokens * batch;
}

WVA_HD double decode_time(const Parms &p, double batch) {
  return p.alpha + p.beta * batch;
}

// state-dependent service rate for batch size b in [1, N] (req/ms)
WVA_HD double serv_rate(const Parms &p, int b) {
  return (double)b / (prefill_time(p, (double)b) + p.num_decode * decode_time(p, (double)b));
}

// log(mu(state n)) for the birth-death recursion, n in [0, K-1]
WVA_HD double log_mu(const Parms &p, int n) {
  int b = n + 1;
  if (b > p.max_batch) b = p.max_batch;
  return log(serv_rate(p, b));
}

WVA_HD bool within_tolerance(double x, double value, double tolerance) {
  if (x == value) return true;
  if (value == 0.0 || tolerance < 0.0) return false;
  return fabs((x - value) / value) <= tolerance;
}

// effective concurrency: solve the service-time identity for n, clamped
WVA_HD double effective_concurrency(const Parms &p, double avg_serv_time) {
  double tokens = (double)(p.out_tokens - 1);
  double numer = avg_serv_time - (p.gamma + p.alpha * tokens);
  double denom = p.delta * p.in_tokens + p.beta * tokens;
  if (denom == 0.0) return numer > 0.0 ? (double)p.max_batch : 0.0;
  double n = numer / denom;
  if (n < 0.0) n = 0.0;
  if (n > (double)p.max_batch) n = (double)p.max_batch;
  return n;
}

struct Stats {
  double throughput;  // req/ms
  double wait;        // ms
  double serv;        // ms
  double n_serv;      // avg requests in service
  // the normalisation, for the waiting-time tail alone: state n has
  // probability exp(logp(n) - log_ref) / (accept_mass + e_K), and an accepted
  // arrival sees it with probability exp(logp(n) - log_ref) / accept_mass
  double accept_mass;  // S - e_K: the states 0..K-1, relative to e^log_ref
  double log_ref;      // m, set by the evaluator that chose it
};

// Mode of the log-probability curve logp[n] = n*log(lam) - cum[n-1].
// The increment logp[n+1]-logp[n] = log(lam) - log(mu(n)) is nonincreasing
// in n because mu(n) = serv_rate(min(n+1, N)) is nondecreasing, so logp is
// concave and its maximum sits where the increment first turns <= 0:
// an O(log N) search over the monotone service-rate curve instead of an
// O(K) max sweep.  Returns the state index n* in [0, K].
// serv_rate(b) < lam  <=>  b < lam * T(b)  (service time T(b) > 0):
// a multiply instead of the fp64 divide inside the mode bisection
WVA_HD bool rate_below(const Parms &p, int b, double lam) {
  double t = prefill_time(p, (double)b) + p.num_decode * decode_time(p, (double)b);
  return (double)b < lam * t;
}

WVA_HD int log_mode_state(const Parms &p, int K, double lam) {
  // lam >= mu(N)  <=>  N <= lam * T(N): all increments > 0, mode at K
  double tN = prefill_time(p, (double)p.max_batch) +
              p.num_decode * decode_time(p, (double)p.max_batch);
  if ((double)p.max_batch <= lam * tN) return K;
  // lam <= mu(1)  <=>  lam * T(1) <= 1: mode at 0
  double t1 = prefill_time(p, 1.0) + p.num_decode * decode_time(p, 1.0);
  if (lam * t1 <= 1.0) return 0;
  // smallest b in [1, N] with serv_rate(b) >= lam; mode = b - 1
  int lo = 1, hi = p.max_batch;
  while (lo < hi) {
    int mid = (lo + hi) / 2;
    if (rate_below(p, mid, lam)) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo - 1;
}

WVA_HD double log_p(const double *cum, double loglam, int n) {
  return (n == 0) ? 0.0 : n * loglam - cum[n - 1];
}

// States more than kLogCutoff nats below the mode contribute < ~1e-16 to
// any normalized sum (at most K * e^-45 relative mass); since logp is
// concave, the significant window [lo, hi] around the mode is found by
// two O(log K) bisections instead of sweeping all K+1 states.
constexpr double kLogCutoff = 45.0;

WVA_HD void state_window(const double *cum, double loglam, int K, int n_star,
                         double m, int *lo_out, int *hi_out) {
  const double thresh = m - kLogCutoff;
  // left edge: logp nondecreasing on [0, n_star]; first n with logp >= thresh
  int lo = 0, hi = n_star;
  while (lo < hi) {
    int mid = (lo + hi) / 2;
    if (log_p(cum, loglam, mid) < thresh) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  *lo_out = lo;
  // right edge: logp nonincreasing on [n_star, K]; last n with logp >= thresh
  lo = n_star;
  hi = K;
  while (lo < hi) {
    int mid = (lo + hi + 1) / 2;
    if (log_p(cum, loglam, mid) < thresh) {
      hi = mid - 1;
    } else {
      lo = mid;
    }
  }
  *hi_out = lo;
}

// Closed-form geometric tail of the state sums (the "queue region").
//
// For n >= N-1 the service rate is constant (mu(n) = serv_rate(N)), so
// consecutive log-probabilities differ by the constant d = log(lam) -
// log(mu_N) and the normalized probabilities e^{logp(n)-m} form a
// geometric sequence.  Summing states [g_start, n_hi] (g_start > N, so
// none of them contribute to the <=N partial sums) in closed form
// replaces up to 10*N per-state exp() calls — the dominant fp64 cost of
// an evaluation — with a handful of exp/expm1.
//
//   S_geo  = p_a * G0,            G0 = sum_{j=0..M} r^j = expm1((M+1)d)/expm1(d)
//   Ni_geo = p_a * (a*G0 + G1),   G1 = sum_{j=0..M} j r^j
//                                    = r (1 - (M+1) r^M + M r^{M+1}) / (1-r)^2
//
// Near r == 1 the G1 numerator cancels; |d|*(M+1) < 0.01 falls back to
// the term-wise loop (a one-or-two-iterate sliver of the bisection).
struct GeoTail {
  double S, Ni, eK;
  bool used;
};

// x_a = log_p(g_start) - m is the first term's exponent; the caller takes it
// from its table (a full table reads an entry, a compact one has none).
WVA_HD GeoTail geo_tail(double x_a, double d, int g_start, int n_hi, int K) {
  GeoTail t{0.0, 0.0, 0.0, false};
  const int M = n_hi - g_start;
  if (M < 8 || fabs(d) * (double)(M + 1) < 0.01) return t;  // loop is fine/safer
  const double p_a = exp(x_a);
  const double e1 = expm1(d);
  const double G0 = expm1((double)(M + 1) * d) / e1;
  const double r = e1 + 1.0;
  const double rM = exp((double)M * d);
  const double G1 =
      r * (1.0 - (double)(M + 1) * rM + (double)M * rM * r) / (e1 * e1);
  t.S = p_a * G0;
  t.Ni = p_a * ((double)g_start * G0 + G1);
  if (n_hi == K) t.eK = p_a * exp((double)(K - g_start) * d);
  t.used = true;
  return t;
}

// Stats from the reduced state sums: the closing arithmetic of every model
// evaluation, host and device
WVA_HD Stats stats_of_sums(double lam, int num, double S, double Ni, double Snum,
                           double Ninum, double eK) {
  Stats st;
  st.accept_mass = S - eK;
  st.log_ref = 0.0;
  st.throughput = lam * (1.0 - eK / S);
  double n_sys = Ni / S;
  st.n_serv = Ninum / S + (1.0 - Snum / S) * (double)num;
  if (st.throughput == 0.0) {
    st.wait = st.serv = 0.0;
  } else {
    double resp = n_sys / st.throughput;
    st.serv = st.n_serv / st.throughput;
    st.wait = resp - st.serv;
    if (st.wait < 0.0) st.wait = 0.0;
  }
  return st;
}

// Scalar model evaluation at arrival rate lam (req/ms) given the inclusive
// cumulative sum cum[n] = sum_{i<=n} log_mu(i), n in [0, K-1].
WVA_HD Stats eval_model(const Parms &p, const double *cum, int K, double lam) {
  double loglam = log(lam);
  // max of logp over n = 0..K via the concavity closed form
  int n_star = log_mode_state(p, K, lam);
  double m = log_p(cum, loglam, n_star);
  if (m < 0.0) m = 0.0;  // logp(0) = 0 participates in the max
  int n_lo, n_hi;
  state_window(cum, loglam, K, n_star, m, &n_lo, &n_hi);
  int num = p.max_batch;  // serv_rate array length
  double S = 0.0, Ni = 0.0, Snum = 0.0, Ninum = 0.0, eK = 0.0;
  // geometric tail over the constant-rate queue region (states > N)
  const int g_start = (num + 1 > n_lo) ? num + 1 : n_lo;
  GeoTail tail{0.0, 0.0, 0.0, false};
  int loop_hi = n_hi;
  if (g_start + 8 <= n_hi) {  // also keeps cum[g_start] in bounds
    const double d = loglam - (cum[g_start] - cum[g_start - 1]);
    tail = geo_tail(log_p(cum, loglam, g_start) - m, d, g_start, n_hi, K);
    if (tail.used) loop_hi = g_start - 1;
  }
  for (int n = n_lo; n <= loop_hi; ++n) {
    double e = exp(log_p(cum, loglam, n) - m);
    S += e;
    Ni += n * e;
    if (n <= num) {
      Snum += e;
      Ninum += n * e;
    }
    if (n == K) eK = e;
  }
  S += tail.S;
  Ni += tail.Ni;
  eK += tail.eK;
  Stats st = stats_of_sums(lam, num, S, Ni, Snum, Ninum, eK);
  st.log_ref = m;
  return st;
}

// ---------------------------------------------------------------------------
// Compact table: N doubles instead of K = 11 * N.
//
// For states n >= N-1 the service rate is constant, so with L_N =
// log(serv_rate(N)) = log_mu(p, N-1)
//
//   cum[n] = cum[N-1] + (n - N + 1) * L_N,   n >= N-1,
//
// and an evaluation reads the table proper only in the sweep over the N+1
// pre-batch states and at the mode (which is at most N-1, or K).  Everything
// past N is closed form: log_p(N+1), log_p(K), and the constant increment
// d = log(lam) - L_N of the geometric tail, taken directly instead of as the
// difference of two table entries of magnitude ~K * |L_N|.  This is the same
// model, not an approximation of it; near saturation it is the more accurate
// of the two, since d no longer cancels.
// ---------------------------------------------------------------------------

// cum[n] for any n in [0, K-1], given cum[0..N-1] and L_N
WVA_HD double cum_at(const double *cum, int N, double log_mu_n, int n) {
  const int i = n < N ? n : N - 1;  // the only index ever read
  const double base = cum[i];
  return n < N ? base : base + (double)(n - N + 1) * log_mu_n;
}

WVA_HD double log_p_compact(const double *cum, int N, double log_mu_n, double loglam,
                            int n) {
  return (n == 0) ? 0.0 : n * loglam - cum_at(cum, N, log_mu_n, n - 1);
}

// The compact table's tail over the whole queue region (N, K], host and
// device: d is taken directly, and *loop_hi is where the term-wise sweep
// stops (N, or K where the tail declines).
WVA_HD GeoTail geo_tail_compact(const double *cum, int N, double log_mu_n, double loglam,
                                double m, int *loop_hi) {
  const int K = N * (1 + kMaxQueueToBatchRatio);
  const int g_start = N + 1;
  const double d = loglam - log_mu_n;
  const GeoTail tail = geo_tail(
      log_p_compact(cum, N, log_mu_n, loglam, g_start) - m, d, g_start, K, K);
  *loop_hi = tail.used ? N : K;
  return tail;
}

// eval_model over the compact table cum[0..N-1] (same inclusive sum), with
// log_mu_n = log_mu(p, N-1).  No significance window: the sweep covers the
// N+1 pre-batch states and the queue region (N, K] sums in closed form; only
// where geo_tail declines (|d| * 10N < 0.01, a sliver around lam = mu(N))
// does the loop run on to K through cum_at.
WVA_HD Stats eval_model_compact(const Parms &p, const double *cum, double log_mu_n,
                                double lam) {
  const int num = p.max_batch;
  const int K = num * (1 + kMaxQueueToBatchRatio);
  const double loglam = log(lam);
  const int n_star = log_mode_state(p, K, lam);  // in [0, N-1], or K
  double m = log_p_compact(cum, num, log_mu_n, loglam, n_star);
  if (m < 0.0) m = 0.0;  // logp(0) = 0 participates in the max
  int loop_hi;
  const GeoTail tail = geo_tail_compact(cum, num, log_mu_n, loglam, m, &loop_hi);
  double S = 0.0, Ni = 0.0, Snum = 0.0, Ninum = 0.0, eK = 0.0;
  for (int n = 0; n <= loop_hi; ++n) {
    double e = exp(log_p_compact(cum, num, log_mu_n, loglam, n) - m);
    S += e;
    Ni += n * e;
    if (n <= num) {
      Snum += e;
      Ninum += n * e;
    }
    if (n == K) eK = e;
  }
  S += tail.S;
  Ni += tail.Ni;
  eK += tail.eK;
  Stats st = stats_of_sums(lam, num, S, Ni, Snum, Ninum, eK);
  st.log_ref = m;
  return st;
}

WVA_HD double eval_ttft_of(const Parms &p, const Stats &st) {
  double effc = effective_concurrency(p, st.serv);
  return st.wait * p.wait_scale + prefill_time(p, effc);
}

WVA_HD double eval_itl_of(const Parms &p, const Stats &st) {
  double effc = effective_concurrency(p, st.serv);
  return decode_time(p, effc);
}

// ---------------------------------------------------------------------------
// Waiting-time tail: P(W > t) of an accepted arrival, from the same chain.
//
// An accepted arrival sees state n with probability pi_n = p[n] / (1 - p[K])
// (Poisson arrivals see time averages).  It waits only when n >= N, and then
// for j = n - N + 1 departures at the constant full-batch rate mu_N =
// serv_rate(N): W | n ~ Erlang(j, mu_N).  With x = mu_N * t and J = K - N,
//
//   P(W > t) = sum_{n=N..K-1} pi_n * sum_{i<j} e^-x x^i / i!.
//
// The states past N are geometric with ratio r = lam / mu_N, d = ln r < 0 on
// the whole search bracket (lam_max = mu_N * (1 - kEpsilon)).  Swapping the
// two sums leaves one sum of J terms,
//
//   P(W > t) = pi_N * sum_{i=0..J-1} T_i / expm1(d),
//   T_i = exp(i * ln(x r) - x - lf[i]) * expm1((J - i) * d),   lf[i] = ln i!,
//
// i.e. Poisson(nu = x r = lam t) weights times g_i = (1 - r^(J-i)) / (1 - r),
// which falls from at most J at i = 0 to 1 at i = J - 1.
//
// Window.  Only the terms within h of c = min(floor(nu), J - 1) are summed.
// Against T_c (a term of the sum, so T_c <= sum), with L = ln(2e16) + 2 ln J:
//   - left, i = c - s: the weights' ratio is prod_{k=i+1..c} k / nu <=
//     prod_{q<s} (1 - q / c) <= exp(-s (s - 1) / (2 c)) because c <= nu, and
//     g_i / g_c <= J; s > h >= sqrt(2 L c) makes every such term at most
//     J e^-L T_c, and there are fewer than J of them: 0.5e-16 T_c in all;
//   - right, i = c + s (only when c = floor(nu)): the ratio is
//     prod_{k=c+1..i} nu / k <= prod_{q<s} 1 / (1 + q / (c + 1)) <=
//     exp(-s (s - 1) / (2 (c + s))) (the Bernstein form of the Poisson upper
//     tail), g_i <= g_c, and h = 2 L + 1 + sqrt(2 L c) gives s (s - 1) >=
//     2 L (c + s) for every s > h: at most J e^-L T_c in all.
// So what the window drops stays below 1e-16 of the sum.  Near saturation at
// N = 700 it keeps about 2000 of the 7000 terms, elsewhere far fewer.
// ---------------------------------------------------------------------------

// The uniform scalars of one tail sum: every thread that shares an
// evaluation computes the same ones.
struct TailSweep {
  bool certain;  // t <= 0: P(W > t) = 1, nothing to sum
  double a;      // ln(x r)
  double log_c;  // ln(pi_N) - x
  double d;      // ln r
  int J;         // terms of the whole sum
  int lo, hi;    // the window: terms lo..hi
  int c;         // the window's centre term, min(floor(nu), J - 1)
  double nu;     // lam t = x r, the Poisson mean (read by the recurrence alone)
};

// st is the mean-model evaluation at lam and logp_n its log_p(N) (every table
// holds cum[N-1]); t follows the contract above.
WVA_HD TailSweep tail_sweep_of(const Parms &p, const Stats &st, double logp_n, double lam,
                               double target_ttft) {
  TailSweep w{true, 0.0, 0.0, 0.0, 0, 0, -1};
  const double t =
      (target_ttft - prefill_time(p, effective_concurrency(p, st.serv))) / p.wait_scale;
  if (!(t > 0.0)) return w;
  w.certain = false;
  const double mu_n = serv_rate(p, p.max_batch);
  const double x = mu_n * t;
  w.d = log(lam) - log(mu_n);
  w.a = log(x) + w.d;
  w.log_c = logp_n - st.log_ref - log(st.accept_mass) - x;
  w.J = p.max_batch * kMaxQueueToBatchRatio;
  const double top = (double)(w.J - 1);
  w.nu = lam * t;  // nu = x r = lam t
  const double c = floor(fmin(w.nu, top));
  const double L = 37.54 + 2.0 * log((double)w.J);
  const double h = 2.0 * L + 1.0 + sqrt(2.0 * L * c);
  w.lo = (int)fmax(c - h, 0.0);
  w.hi = (int)fmin(c + h, top);
  w.c = (int)c;
  return w;
}

// The tail sum given a log-factorial accessor lf(i) = ln i!: the window's
// terms lo + first, lo + first + stride, ... (first = 0, stride = 1 is the
// whole window; a workgroup's threads take first = tid, stride = THREADS and
// add their results).  Two independent exp / expm1 chains per pass, as in the
// mean model's sweep.  Every expm1 factor is negative: the result is <= 0.
template <typename LogFact>
WVA_HD double tail_sum(const TailSweep &w, const LogFact &lf, int first, int stride) {
  double s0 = 0.0, s1 = 0.0;
  int i = w.lo + first;
  for (; i + stride <= w.hi; i += 2 * stride) {
    const int i2 = i + stride;
    const double e = exp((double)i * w.a - lf(i) + w.log_c);
    const double e2 = exp((double)i2 * w.a - lf(i2) + w.log_c);
    s0 += e * expm1((double)(w.J - i) * w.d);
    s1 += e2 * expm1((double)(w.J - i2) * w.d);
  }
  if (i <= w.hi) {
    s0 += exp((double)i * w.a - lf(i) + w.log_c) * expm1((double)(w.J - i) * w.d);
  }
  return s0 + s1;
}

// P(W > t) from the reduced tail sum; the clamp only trims rounding
WVA_HD double tail_probability(const TailSweep &w, double sum) {
  return fmin(fmax(sum / expm1(w.d), 0.0), 1.0);
}

// ---------------------------------------------------------------------------
// The tail sum without a log-factorial table: the Poisson weights by their
// recurrence, over contiguous chunks.  Same model, same window, same result up
// to rounding; it needs no memory besides the cumulative table, so it holds
// any N the compact table holds.
//
// With e(i) = i a - lf(i) + log_c the term is T_i = exp(e(i)) expm1((J-i) d).
// The window lo..hi is cut into `parts` contiguous chunks of ceil(window /
// parts) terms, the last short or empty; a workgroup thread takes chunk tid,
// the host the one chunk.  A worker forms the weight of its chunk's first
// term once, relative to the centre term c of the window,
//
//   w_i0 = exp(e(i0) - e(c)) = exp((i0 - c) a - (lf(i0) - lf(c))),
//
// with lf from the closed form below, and then walks
//
//   w_{i+1} = w_i nu / (i + 1),   sum += w_i expm1((J - i) d):
//
// one expm1 and one multiply-divide per term, no exp, no table read.  The
// reduced sum is scaled back by exp(e(c)) (tail_centre_term) before
// tail_probability.  log_c (ln pi_N - x, as small as it likes) enters only
// there: inside the window the relative weights lie between about e^-2L
// (window bound above, L ~ 60) and 1, so none underflows or overflows however
// small pi_N is.
//
// Error.  The chunk's first weight carries the rounding of two lf values and
// of (i0 - c) a, about 2^-53 (lf(i0) + lf(c) + |i0 - c| a): 2e-10 relative at
// J = 76800, what the scanned table's entries carry as well.  Each recurrence
// step adds three roundings (the stride-2 form below), so a chunk of n terms
// drifts by at most 1.5 n 2^-52: 25 terms per thread at N = 7680 near
// saturation (a window of ~6300 terms over 256 threads) is 1e-14, and the
// host's single chunk of 6300 is 2e-12.  Both stay far inside the search's
// 1e-6 stop and below the first weight's own error.
// ---------------------------------------------------------------------------

// lf(i) = ln i!, i >= 0, without a table to scan.  Below 16 the correctly
// rounded values; from 16 on the Stirling series
//   (i + 1/2) ln i - i + ln(2 pi) / 2 + 1/(12 i) - 1/(360 i^3) + 1/(1260 i^5)
//   - 1/(1680 i^7) + 1/(1188 i^9).
// For a positive argument the series alternates around the true value, so the
// truncation error is below the first omitted term, 691 / (360360 i^11): at
// most 1.1e-16 at i = 16, where 2^-53 lf(i) = 3.4e-15, and the ratio falls
// like i^-12 from there.  Measured against 60-digit values for every i <
// 3000 and every 7th up to 80000, the whole error, rounding included, stays
// within 3.5e-16 lf(i).  lgamma(i + 1) was the alternative: the host's is no
// more accurate on the same values (5.1e-16 lf(i)), and inlined into the
// compact tail kernel the device library's takes it from 159 to 256 vector
// registers plus 10 AGPRs, that is from 3 waves per SIMD to 1, and from 15.5k
// to 25.3k lines of assembly (cross-compiled for gfx950, not run).
WVA_HD double log_factorial(int i) {
  static constexpr double kSmall[16] = {0.0,
                                 0.0,
                                 0.6931471805599453,
                                 1.791759469228055,
                                 3.1780538303479458,
                                 4.787491742782046,
                                 6.579251212010101,
                                 8.525161361065415,
                                 10.60460290274525,
                                 12.801827480081469,
                                 15.104412573075516,
                                 17.502307845873887,
                                 19.987214495661885,
                                 22.552163853123425,
                                 25.19122118273868,
                                 27.89927138384089};
  if (i < 16) return kSmall[i < 0 ? 0 : i];
  const double x = (double)i;
  const double r = 1.0 / x;
  const double r2 = r * r;
  const double series =
      r * (1.0 / 12.0 +
           r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0)))));
  return (x + 0.5) * log(x) - x + 0.9189385332046727 + series;
}

// exp(e(c)): what the chunked sums are relative to
WVA_HD double tail_centre_term(const TailSweep &w) {
  return exp((double)w.c * w.a - log_factorial(w.c) + w.log_c);
}

// Chunk `part` of `parts` of the window, relative to the centre term.  Two
// independent chains per pass, as in the other sweeps: the even and the odd
// terms of the chunk, each by the recurrence's stride-2 form w_{i+2} = w_i
// nu^2 / ((i + 1)(i + 2)) (the integer product is exact below 2^53).  Every
// expm1 factor is negative: the result is <= 0.  0 for an empty chunk.
WVA_HD double tail_sum_chunk(const TailSweep &w, int part, int parts) {
  const int len = (w.hi - w.lo + parts) / parts;  // ceil(window / parts)
  const int i0 = w.lo + part * len;
  const int end = i0 + len - 1 < w.hi ? i0 + len - 1 : w.hi;
  if (i0 > end) return 0.0;
  const double nu2 = w.nu * w.nu;
  double wa = exp((double)(i0 - w.c) * w.a - (log_factorial(i0) - log_factorial(w.c)));
  double wb = wa * w.nu / (double)(i0 + 1);
  double s0 = 0.0, s1 = 0.0;
  int i = i0;
  for (; i + 1 <= end; i += 2) {
    s0 += wa * expm1((double)(w.J - i) * w.d);
    s1 += wb * expm1((double)(w.J - i - 1) * w.d);
    wa *= nu2 / ((double)(i + 1) * (double)(i + 2));
    wb *= nu2 / ((double)(i + 2) * (double)(i + 3));
  }
  if (i <= end) s0 += wa * expm1((double)(w.J - i) * w.d);
  return s0 + s1;
}

// ---------------------------------------------------------------------------
// TTFT quantile: the inverse of the waiting-time tail.  Given a per-replica
// rate rho (req/s) and a tail probability eps, the TTFT that an accepted
// arrival exceeds with probability eps (eps = 0.05: the p95 TTFT).
//
// With lam = rho / 1000, st the mean-model evaluation at lam, prefill =
// prefill_time(effective_concurrency(st.serv)), J = 10 N, mu_N = serv_rate(N)
// and d = ln lam - ln mu_N:
//   - p_wait = P(W > 0) = sum_{n=N..K-1} pi_n = pi_N expm1(J d) / expm1(d);
//   - p_wait <= eps: nobody waits that often, t = 0;
//   - otherwise t is the root of P(W > t) = eps, found by binary_search over t
//     on [0, t_hi] with y(0) := p_wait and, for t > 0, y(t) the tail sum above
//     (same window, same tail_probability);
//   - q = wait_scale * t + prefill, in ms.
// Lambda is fixed, so st, pi_N, d and the weights expm1((J - i) d) are
// constants of the row: only the Poisson part of a term moves with t.
//
// Bracket.  Given the state, the wait is Erlang(j, mu_N) with j <= J, which is
// stochastically below Erlang(J, mu_N), so P(W > t) <= P(Gamma(J, 1) > mu_N t).
// Laurent-Massart: P(Gamma(J, 1) >= J + sqrt(2 J l) + l) <= e^-l.  With l =
// ln(2 / eps) and t_hi = (J + sqrt(2 J l) + l) / mu_N this is P(W > t_hi) <=
// eps / 2: the target lies strictly inside [0, t_hi] and is never within the
// search's tolerance of its upper end.  (ln(2 / eps), not ln(1 / eps): p_wait
// can be 1 - 1e-30 at large N, so nothing can be gained from pi.)
//
// The result row has two doubles, (valid, q): q = 0 is a legitimate value (a
// decode-only row with nobody waiting).  (0, 0) for a row that fails
// row_valid, an eps that is no finite number in the open (0, 1) (there is no
// 100th percentile), or a rate that QueueAnalyzer.analyze rejects: NaN, +-inf,
// <= 0, or above lam_max * 1000.
// ---------------------------------------------------------------------------
enum QuantileField { Q_VALID = 0, Q_TTFT, QUANTILE_FIELDS };

// eps and the rate of a VALID row; ordered compares are false for NaN
WVA_HD bool quantile_inputs_valid(const Parms &p, double rate, double eps) {
  const double lam_max = serv_rate(p, p.max_batch) * (1.0 - kEpsilon);
  return (eps > 0.0) & (eps < 1.0) & (rate > 0.0) & (rate <= lam_max * 1000.0);
}

// The constants of one row's search over t: uniform over everything that
// shares the row.
struct QuantileRow {
  double lam;       // req/ms
  double prefill;   // ms, at the mean evaluation's effective concurrency
  double mu_n;      // serv_rate(N)
  double d;         // ln lam - ln mu_N, < 0
  double log_pi_n;  // ln pi_N
  double p_wait;    // P(W > 0)
  double t_hi;      // the bracket's upper end, ms
  int J;
};

// st is the mean-model evaluation at lam and logp_n its log_p(N)
WVA_HD QuantileRow quantile_row_of(const Parms &p, const Stats &st, double logp_n, double lam,
                                   double eps) {
  QuantileRow q;
  q.lam = lam;
  q.prefill = prefill_time(p, effective_concurrency(p, st.serv));
  q.mu_n = serv_rate(p, p.max_batch);
  q.d = log(lam) - log(q.mu_n);
  q.J = p.max_batch * kMaxQueueToBatchRatio;
  q.log_pi_n = logp_n - st.log_ref - log(st.accept_mass);
  q.p_wait = exp(q.log_pi_n) * (expm1((double)q.J * q.d) / expm1(q.d));
  const double l = log(2.0 / eps);
  q.t_hi = ((double)q.J + sqrt(2.0 * (double)q.J * l) + l) / q.mu_n;
  return q;
}

// tail_sweep_of for a given t > 0 instead of a TTFT target: the same scalars
// and the same window rule
WVA_HD TailSweep tail_sweep_at(const QuantileRow &q, double t) {
  TailSweep w{false, 0.0, 0.0, 0.0, 0, 0, -1};
  const double x = q.mu_n * t;
  w.d = q.d;
  w.a = log(x) + w.d;
  w.log_c = q.log_pi_n - x;
  w.J = q.J;
  const double top = (double)(w.J - 1);
  w.nu = q.lam * t;
  const double c = floor(fmin(w.nu, top));
  const double L = 37.54 + 2.0 * log((double)w.J);
  const double h = 2.0 * L + 1.0 + sqrt(2.0 * L * c);
  w.lo = (int)fmax(c - h, 0.0);
  w.hi = (int)fmin(c + h, top);
  w.c = (int)c;
  return w;
}

// the closing arithmetic: from the searched t to the TTFT quantile
WVA_HD double quantile_ttft(const Parms &p, const QuantileRow &q, double t) {
  return p.wait_scale * t + q.prefill;
}

// ---------------------------------------------------------------------------
// y(t) = P(W > t) of a QuantileRow without any table: the quantile search at
// any N the compact table holds.  Window and scalars are tail_sweep_at's, the
// window is cut into `parts` contiguous chunks as in tail_sum_chunk, and the
// result is relative to the centre term in the same way (tail_centre_term).
//
// Lambda is fixed, so the geometric factor expm1((J - i) d) of a term is a
// constant of the row and u_i = exp((J - i) d) a geometric sequence in i with
// the ratio exp(-d) > 1 (quantile_growth, once per row).  A chunk forms u at
// its first term with one exp and carries it along,
//
//   u_{i+2} = u_i exp(-2 d),   T_i = w_i (u_i - 1),
//
// next to the Poisson weight's stride-2 recurrence of tail_sum_chunk: two
// multiply chains, one divide and no transcendental call per term, where
// tail_sum_chunk pays an expm1.
//
// Underflow.  u grows along the chunk, so a first value that has underflowed
// (or is denormal) would leave u = 0 at terms where the true u_i is not
// negligible.  The chain is therefore taken only where (J - i0) |d| <=
// kChainMaxExponent = 690: u_i0 >= e^-690 = 2e-300 is a normal number, every
// later u_i is larger, and none exceeds u_{J-1} = e^d < 1 where it is read
// (the value carried past the chunk's last term is at most e^{-2d} u_{J-1},
// finite because a chunk that takes a step has J - i0 >= 2, that is 2 |d| <=
// 690).  Any other chunk is tail_sum_chunk's, expm1 per term.
//
// Error.  Both chains take one step per two terms.  The longest chunk is the
// host's and the kernel's alike, ceil(window / 64): the window has at most 2 h
// + 1 = 6315 terms at J = 76800 (tail_sweep_at), so 99 terms and 50 steps.
//   - The weight chain is tail_sum_chunk's: three roundings per step, 1.5 n
//     2^-52 = 3.3e-14 over 99 terms, behind the first weight's 2e-10.
//   - u: the first value carries exp's rounding and that of its argument,
//     (J - i0) |d| 2^-53; a step multiplies by exp(-d)^2, a constant known to
//     3 roundings, and rounds once: 4 2^-53 per step, 2.2e-14 over 50 steps.
//   - u - 1 cancels.  Every valid rate has |d| >= -ln(1 - kEpsilon) = 1.0005e-3
//     (lam <= mu_N (1 - kEpsilon)), and J - i >= 1 inside the window, so 1 -
//     u_i >= 1 - e^-|d| >= 1e-3 and a relative error delta of u_i becomes
//     delta u_i / (1 - u_i) <= delta / ((J - i) |d|) <= 1000 delta in the
//     term.  For the drift and exp's rounding that is 1000 (2.2e-14 + 2.2e-16)
//     = 2.3e-11.  The argument's share, (J - i0) |d| 2^-53 / ((J - i) |d|), is
//     at most 100 2^-53 = 1.1e-14, since J - i0 <= 100 (J - i) over a chunk of
//     99 terms.
// Every term has the same sign, so the sum's relative error is at most the
// worst term's, 2.3e-11: five orders inside the search's 1e-6 stop on y, and
// below the first weight's own 2e-10.
// ---------------------------------------------------------------------------
constexpr double kChainMaxExponent = 690.0;

// exp(-d): the ratio of the u chain, a constant of the row
WVA_HD double quantile_growth(const QuantileRow &q) { return exp(-q.d); }

// Chunk `part` of `parts` of the window, relative to the centre term; growth
// is quantile_growth of the row w was made for.  <= 0; 0 for an empty chunk.
WVA_HD double quantile_sum_chunk(const TailSweep &w, double growth, int part, int parts) {
  const int len = (w.hi - w.lo + parts) / parts;  // ceil(window / parts)
  const int i0 = w.lo + part * len;
  const int end = i0 + len - 1 < w.hi ? i0 + len - 1 : w.hi;
  if (i0 > end) return 0.0;
  const double reach = (double)(w.J - i0) * w.d;  // ln u_i0, < 0
  if (reach < -kChainMaxExponent) return tail_sum_chunk(w, part, parts);
  const double nu2 = w.nu * w.nu;
  const double growth2 = growth * growth;
  double wa = exp((double)(i0 - w.c) * w.a - (log_factorial(i0) - log_factorial(w.c)));
  double wb = wa * w.nu / (double)(i0 + 1);
  double ua = exp(reach);
  double ub = ua * growth;
  double s0 = 0.0, s1 = 0.0;
  int i = i0;
  for (; i + 1 <= end; i += 2) {
    s0 += wa * (ua - 1.0);
    s1 += wb * (ub - 1.0);
    wa *= nu2 / ((double)(i + 1) * (double)(i + 2));
    wb *= nu2 / ((double)(i + 2) * (double)(i + 3));
    ua *= growth2;
    ub *= growth2;
  }
  if (i <= end) s0 += wa * (ua - 1.0);
  return s0 + s1;
}

// The chunks one wave's lanes take, and the host sums in sequence
constexpr int kQuantileChunks = 64;

// Whether an evaluator offers exceedance(lam, target_ttft) = P(TTFT > target)
// next to eval(lam); one that does not sizes to the mean TTFT alone, and the
// callers route no row with ttft_tail > 0 to it.
template <typename Ev>
constexpr auto has_exceedance(int) -> decltype((void)((const Ev *)nullptr)->exceedance(0.0, 0.0),
                                               true) {
  return true;
}
template <typename Ev>
constexpr bool has_exceedance(long) {
  return false;
}

// ---------------------------------------------------------------------------
// Occupancy tail: the share of tokens whose ITL exceeds a target, from the
// same chain.
//
// A decode step with b = min(n, N) requests in service takes decode_time(b),
// and every token it emits has that inter-token latency.  In state n the chain
// completes requests at rate mu(n), so tokens are emitted in proportion to
// p[n] mu(n), and the share of tokens slower than target_itl is
//
//   y(lam) = sum_{n=1..K, decode_time(min(n,N)) > target} p[n] mu(n)
//            / sum_{n=1..K} p[n] mu(n).
//
// decode_time is non-decreasing in b, so the batch sizes that meet the target
// are a prefix 1..c, c = itl_threshold_count.  Detailed balance, p[n] mu(n) =
// lam p[n-1], turns both sums into sums of state probabilities, and the
// denominator into the throughput lam (1 - p[K]):
//
//   y(lam) = 0                                   if c = N,
//   y(lam) = sum_{j=c..K-1} pi_j,  pi_j = p[j] / (1 - p[K])   otherwise:
//
// the probability that an accepted arrival finds at least c requests in the
// system (1 for c = 0).  The chain is stochastically increasing in lam, so y
// is non-decreasing and binary_search runs on it over rate_bracket unchanged.
//
// Evaluation over the compact table, relative to e^m as in eval_model_compact:
//   - the upper mass U = sum_{j=c..N} exp(log_p(j) - m) and the whole
//     pre-batch mass A = sum_{j=0..N} exp(log_p(j) - m), term by term;
//   - G, the states N+1..K-1 (not K), by geo_tail.  It never declines here:
//     an evaluation happens only for 0 < c < N, so N >= 2, and on the bracket
//     |d| >= -ln(1 - kEpsilon) = 1.0005e-3, so (10 N - 1) |d| >= 0.019 > 0.01;
//   - y = (U + G) / (A + G).  U is summed directly, all terms positive: 1 -
//     sum_{j<c} pi_j would cancel exactly where eps is small.
// No Ni / Ninum moments, no effective concurrency.
// ---------------------------------------------------------------------------

// c = #{b in 1..N : decode_time(b) <= target_itl}: the last b that meets the
// target, by bisection on the predicate every implementation shares.
WVA_HD int itl_threshold_count(const Parms &p, double target_itl) {
  int lo = 0, hi = p.max_batch;  // decode_time(lo) meets the target (or lo = 0)
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (decode_time(p, (double)mid) <= target_itl) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

// The uniform scalars of one occupancy-tail evaluation: every thread that
// shares it computes the same ones.
struct OccupancySweep {
  double loglam, m;  // log(lam) and the log reference, max(log_p(mode), 0)
  double geo;        // G: the states N+1..K-1
};

WVA_HD OccupancySweep occupancy_sweep_of(const Parms &p, const double *cum, double log_mu_n,
                                         double lam) {
  const int N = p.max_batch;
  const int K = N * (1 + kMaxQueueToBatchRatio);
  OccupancySweep w;
  w.loglam = log(lam);
  w.m = log_p_compact(cum, N, log_mu_n, w.loglam, log_mode_state(p, K, lam));
  if (w.m < 0.0) w.m = 0.0;
  const GeoTail tail = geo_tail(log_p_compact(cum, N, log_mu_n, w.loglam, N + 1) - w.m,
                                w.loglam - log_mu_n, N + 1, K - 1, K);
  w.geo = tail.S;  // tail.used: N >= 2 and lam inside rate_bracket (above)
  return w;
}

// Both mass sums over the states first, first + stride, ... <= N (first =
// 0, stride = 1 is the whole sweep; a workgroup's threads take first = tid,
// stride = THREADS and add their results).  Two independent exp chains per
// pass, as in the mean model's sweep.
WVA_HD void occupancy_sums(const OccupancySweep &w, const double *cum, int N, double log_mu_n,
                           int c, int first, int stride, double *all, double *upper) {
  double a0 = 0.0, a1 = 0.0, u0 = 0.0, u1 = 0.0;
  int n = first;
  for (; n + stride <= N; n += 2 * stride) {
    const int n2 = n + stride;
    const double e = exp(log_p_compact(cum, N, log_mu_n, w.loglam, n) - w.m);
    const double e2 = exp(log_p_compact(cum, N, log_mu_n, w.loglam, n2) - w.m);
    a0 += e;
    a1 += e2;
    u0 += n >= c ? e : 0.0;
    u1 += n2 >= c ? e2 : 0.0;
  }
  if (n <= N) {
    const double e = exp(log_p_compact(cum, N, log_mu_n, w.loglam, n) - w.m);
    a0 += e;
    u0 += n >= c ? e : 0.0;
  }
  *all = a0 + a1;
  *upper = u0 + u1;
}

// y from the reduced sums; the clamp only trims rounding
WVA_HD double occupancy_tail(const OccupancySweep &w, double all, double upper) {
  return fmin(fmax((upper + w.geo) / (all + w.geo), 0.0), 1.0);
}

// ---------------------------------------------------------------------------
// ITL quantile: the inverse of the occupancy tail at a fixed rate.  Given a
// per-replica rate rho (req/s) and a token share eps, the ITL that a fraction
// eps of the tokens exceeds (eps = 0.05: the p95 ITL).
//
// With lam = rho / 1000 and, for a batch count b in 1..N, S_b the share of
// tokens emitted in decode steps with MORE than b requests in service, the
// detailed balance of "Occupancy tail" gives
//
//   S_b = sum_{j=b..K-1} pi_j,  pi_j = p[j] / (1 - p[K]),  b < N;   S_N = 0,
//
// non-increasing in b, and
//
//   b*    = min { b in 1..N : S_b <= eps },
//   q_itl = decode_time(b*) = alpha + beta * b*.
//
// It is stated on the batch index, not on a comparison of decode times, so
// beta = 0 and N = 1 are no special cases of the definition (both give alpha +
// beta).  The wait scale plays no part: occupancy does not depend on it.
//
// Evaluation.  lam is fixed, so this is the inverse of a step function: ONE
// sweep over the pre-batch states and a scan, not a search.  Relative to e^m
// (occupancy_sweep_of), with e_j = exp(log_p(j) - m), G the states N+1..K-1
// and A = sum_{j=0..N} e_j,
//
//   T_b = G + sum_{j=b..N} e_j,   S_b = T_b / (A + G) for b < N,
//
// and with b_f the last b in 0..N-1 whose T_b exceeds eps (A + G) (b_f = 0 at
// least: T_0 = A + G and eps < 1), b* = max(b_f + 1, 1): itl_quantile_batch.
// T is summed directly from the top, all terms positive, never as 1 - prefix,
// for the reason given under "Occupancy tail".  b* = N needs no S at all, so
// N = 1 evaluates nothing; that is also what keeps geo_tail from declining
// (N >= 2 and lam <= lam_max give (10 N - 1) |d| >= 0.019, as above; at N = 1
// it would decline near lam_max).
//
// The result row is that of the TTFT quantile, (valid, q), under the same
// rules without a cs^2: (0, 0) for a row that fails row_valid, an eps that is
// no finite number in the open (0, 1), or a rate that is NaN, +-inf, <= 0 or
// above lam_max * 1000 (quantile_inputs_valid).
// ---------------------------------------------------------------------------
constexpr int Q_ITL = Q_TTFT;  // column 1 of an ITL quantile row

// e_j of a sweep
WVA_HD double occupancy_term(const OccupancySweep &w, const double *cum, int N, double log_mu_n,
                             int j) {
  return exp(log_p_compact(cum, N, log_mu_n, w.loglam, j) - w.m);
}

// b* from b_f, the last state whose suffix mass exceeds eps (A + G).  A b_f
// of N (T_N = G + e_N is a mass, not S_N = 0) means b* = N like N - 1 does,
// and -1 (nothing above, which only rounding could produce) means 1.
WVA_HD int itl_quantile_batch(int last_above, int N) {
  const int b = last_above + 1;
  return b < 1 ? 1 : (b > N ? N : b);
}

// The serial host reference: b* of a valid row at lam (req/ms) over the
// compact table.  One sweep from the top, the running suffix mass starting
// from G and stored for the states below N (suffix must hold N doubles), then
// a bisection over the stored values, which never decrease towards 0 (adding
// a positive term never lowers a rounded sum).
inline int itl_quantile_row(const Parms &p, const double *cum, double log_mu_n, double lam,
                            double eps, double *suffix) {
  const int N = p.max_batch;
  if (N == 1) return 1;
  const OccupancySweep w = occupancy_sweep_of(p, cum, log_mu_n, lam);
  double run = w.geo;
  for (int j = N; j >= 0; --j) {
    run += occupancy_term(w, cum, N, log_mu_n, j);
    if (j < N) suffix[j] = run;
  }
  const double thresh = eps * run;  // eps (A + G)
  // first j in [0, N] with suffix[j] <= thresh (N: none); b_f is the one before
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (suffix[mid] > thresh) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return itl_quantile_batch(lo - 1, N);
}

// Whether an evaluator offers itl_exceedance(lam, c) next to eval(lam), and
// itl_eps(), the row's itl_tail; one that does not sizes to the mean ITL alone,
// and the callers route no row with itl_tail > 0 to it.
template <typename Ev>
constexpr auto has_itl_exceedance(int)
    -> decltype((void)((const Ev *)nullptr)->itl_exceedance(0.0, 0), true) {
  return true;
}
template <typename Ev>
constexpr bool has_itl_exceedance(long) {
  return false;
}

// ---------------------------------------------------------------------------
// Monotone bisection mirroring analyzer/search.py: boundary classification
// -1 below / 0 within / +1 above, relative tolerance, 100 iterations.
// ---------------------------------------------------------------------------

constexpr int kBisect = 2;  // classify_bracket: the target lies strictly inside

// Classifies a bracket from its two end values y0 = y(x_min), y1 = y(x_max).
// Returns the indicator with *x_star set, or kBisect with *increasing set.
WVA_HD int classify_bracket(double x_min, double x_max, double y0, double y1,
                            double y_target, double *x_star, bool *increasing) {
  if (within_tolerance(y0, y_target, kTolerance)) {
    *x_star = x_min;
    return 0;
  }
  if (within_tolerance(y1, y_target, kTolerance)) {
    *x_star = x_max;
    return 0;
  }
  if (within_tolerance(y0, y1, kTolerance)) {
    // flat function: classify by value only (direction would be noise)
    if (y_target > fmax(y0, y1)) {
      *x_star = x_max;
      return +1;
    }
    *x_star = x_min;
    return -1;
  }
  *increasing = y0 < y1;
  if ((*increasing && y_target < y0) || (!*increasing && y_target > y0)) {
    *x_star = x_min;
    return -1;
  }
  if ((*increasing && y_target > y1) || (!*increasing && y_target < y1)) {
    *x_star = x_max;
    return +1;
  }
  return kBisect;
}

// Both bracket ends are evaluated before anything is classified, as the
// speculative search does.  Earlier sequential searches returned after
// y(x_min) when it already met the target within the tolerance; such a row
// now costs one evaluation more and gets the same answer, because the
// classification tests y0 first.
// On the device every thread that shares an evaluator runs this in lockstep:
// the eval results are identical on all of them because they come from
// broadcast reductions, so the control flow is uniform.
template <typename F>
WVA_HD int binary_search(double x_min, double x_max, double y_target, F eval,
                         double *x_star) {
  const double y0 = eval(x_min);
  const double y1 = eval(x_max);
  bool increasing = false;
  const int ind = classify_bracket(x_min, x_max, y0, y1, y_target, x_star, &increasing);
  if (ind != kBisect) return ind;
  double xs = x_min;
  for (int i = 0; i < kMaxIterations; ++i) {
    xs = 0.5 * (x_min + x_max);
    double ys = eval(xs);
    if (within_tolerance(ys, y_target, kTolerance)) break;
    // (spelled out, here and in the speculative walk: behind a helper the
    // compiler no longer specialises the loop on `increasing`, and the
    // 256-thread kernels lose a wave per SIMD to the extra registers)
    if ((increasing && y_target < ys) || (!increasing && y_target > ys)) {
      x_max = xs;
    } else {
      x_min = xs;
    }
  }
  *x_star = xs;
  return 0;
}

// ---------------------------------------------------------------------------
// Row solve: the non-zero-load body of core.create_allocation over any
// evaluator, i.e. anything with eval(lam) -> Stats (host table, LDS table,
// one wave or a workgroup).  Two parts, so that a kernel that runs the two
// searches its own way can use the second alone.
// ---------------------------------------------------------------------------

// rate range of the searches, req/ms
WVA_HD void rate_bracket(const Parms &p, double *lam_min, double *lam_max) {
  *lam_min = serv_rate(p, 1) * kEpsilon;
  *lam_max = serv_rate(p, p.max_batch) * (1.0 - kEpsilon);
}

// Part 1: the TTFT search, then the ITL search.  False when a target lies
// below the bounded region: the row is infeasible.
template <typename Ev>
WVA_HD bool search_targets(const double *pr, const Parms &p, const Ev &ev, double lam_min,
                           double lam_max, double *lam_ttft, double *lam_itl) {
  *lam_ttft = lam_max;
  if (pr[P_TARGET_TTFT] > 0.0) {
    // the TTFT functional: the tail P(TTFT > target) against eps for a row
    // that carries one, the mean TTFT against the target otherwise
    bool to_percentile = false;
    if constexpr (has_exceedance<Ev>(0)) {
      if (p.tail_eps > 0.0) {
        to_percentile = true;
        auto tail = [&](double lam) { return ev.exceedance(lam, pr[P_TARGET_TTFT]); };
        if (binary_search(lam_min, lam_max, p.tail_eps, tail, lam_ttft) < 0) return false;
      }
    }
    if (!to_percentile) {
      auto ttft = [&](double lam) { return eval_ttft_of(p, ev.eval(lam)); };
      if (binary_search(lam_min, lam_max, pr[P_TARGET_TTFT], ttft, lam_ttft) < 0) return false;
    }
  }
  *lam_itl = lam_max;
  if (pr[P_TARGET_ITL] > 0.0) {
    // the ITL functional: the occupancy tail against eps for a row that
    // carries one, the mean ITL against the target otherwise
    if constexpr (has_itl_exceedance<Ev>(0)) {
      if (ev.itl_eps() > 0.0) {
        const int c = itl_threshold_count(p, pr[P_TARGET_ITL]);
        if (c == 0) return false;               // y = 1 at every rate
        if (c == p.max_batch) return true;      // y = 0 at every rate: lam_max
        auto tail = [&](double lam) { return ev.itl_exceedance(lam, c); };
        return binary_search(lam_min, lam_max, ev.itl_eps(), tail, lam_itl) >= 0;
      }
    }
    auto itl = [&](double lam) { return eval_itl_of(p, ev.eval(lam)); };
    if (binary_search(lam_min, lam_max, pr[P_TARGET_ITL], itl, lam_itl) < 0) return false;
  }
  return true;
}

// One result row by value, in ResultField order; RowValues{} is the all-zero
// row of an infeasible or rejected problem.  Named fields, returned by value
// and not through memory: the kernels pick one field per thread, and values
// that live behind a pointer there end up in scratch memory, not registers.
struct RowValues {
  double feasible, replicas, rate_star, itl, ttft, rho;
};

// Part 2: from the two searched rates (and the TPS back-off) to the result
// row.  Knows nothing about threads: every thread that shares ev runs it and
// gets the same answer.
template <typename Ev>
WVA_HD RowValues row_tail(const double *pr, const Parms &p, const Ev &ev, double lam_max,
                          double lam_ttft, double lam_itl) {
  double lam_tps = lam_max;
  if (pr[P_TARGET_TPS] > 0.0) lam_tps = lam_max * (1.0 - kStabilityFraction);

  const double lam = fmin(lam_ttft, fmin(lam_itl, lam_tps));
  Stats st = ev.eval(lam);
  const double rate_star = st.throughput * 1000.0;  // req/s

  const double total_rate = pr[P_TOTAL_RATE];
  double n_rep = ceil(total_rate / rate_star);
  const double min_rep = trunc(pr[P_MIN_REPLICAS]);
  if (n_rep < min_rep) n_rep = min_rep;
  // no replicas, or a per-replica rate that is not > 0 (zero or negative
  // load; NaN from 0/0 fails every ordered compare): infeasible
  if (!(n_rep > 0.0)) return RowValues{};
  const double rate = total_rate / n_rep;  // req/s per replica
  if (!(rate > 0.0) || rate > lam_max * 1000.0) return RowValues{};

  Stats fin = ev.eval(rate / 1000.0);
  double rho = fin.n_serv / (double)p.max_batch;
  // The kernels' form of the clamp, on the host as well (which used two
  // ifs): a NaN rho comes out as 0 and -0.0 as +0.0, where the ifs passed
  // both through.  A NaN cannot arise here: rate <= lam_max keeps the tail's
  // d negative and every sum finite.
  rho = fmin(fmax(rho, 0.0), 1.0);

  return RowValues{1.0, n_rep, rate_star, eval_itl_of(p, fin), eval_ttft_of(p, fin), rho};
}

// Both parts over one evaluator.
template <typename Ev>
WVA_HD RowValues solve_row(const double *pr, const Parms &p, const Ev &ev) {
  double lam_min, lam_max, lam_ttft, lam_itl;
  rate_bracket(p, &lam_min, &lam_max);
  if (!search_targets(pr, p, ev, lam_min, lam_max, &lam_ttft, &lam_itl)) return RowValues{};
  return row_tail(pr, p, ev, lam_max, lam_ttft, lam_itl);
}

}  // namespace wva
