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
};

// largest N whose chain length (1 + ratio) * N still fits an int
constexpr int kMaxBatchLimit = 2147483647 / (1 + kMaxQueueToBatchRatio);

// The row contract above.  Ordered compares are false for NaN, so each
// test is written to hold only for a proper value.  Branch-free (& rather
// than && or early returns): the kernels run this before anything else,
// and nothing in it should make one load wait for another's compare.
// scv is the row's service-time cs^2 (1.0 when the launch carries none):
// finite and >= 0, so the -1 sentinel never passes.
WVA_HD bool row_valid(const double *pr, double scv = 1.0) {
  bool ok = (scv >= 0.0) & (scv <= 1.7976931348623157e308);
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
WVA_HD Parms parms_from_problem(const double *pr, double scv = 1.0) {
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
  return stats_of_sums(lam, num, S, Ni, Snum, Ninum, eK);
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
  return stats_of_sums(lam, num, S, Ni, Snum, Ninum, eK);
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
    auto ttft = [&](double lam) { return eval_ttft_of(p, ev.eval(lam)); };
    if (binary_search(lam_min, lam_max, pr[P_TARGET_TTFT], ttft, lam_ttft) < 0) return false;
  }
  *lam_itl = lam_max;
  if (pr[P_TARGET_ITL] > 0.0) {
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
