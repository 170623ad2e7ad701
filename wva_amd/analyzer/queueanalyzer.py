"""Inference-server queue analyzer: build, analyze, size.

Parity with /root/reference/pkg/analyzer/queueanalyzer.go:

- service time of a batch of n requests:
    prefill(n) = gamma + delta * inTokens * n       (0 when inTokens == 0)
    decode(n)  = alpha + beta * n
    state-dependent service rate mu(n) = n / (prefill(n) + numDecode*decode(n))
  with numDecode = outTokens-1, special-cased to 1 for decode-only/one-token
  requests (queueanalyzer.go:104-110);
- stable arrival-rate range [eps*mu(1), (1-eps)*mu(N)], eps = 0.001;
- occupancy bound K = maxQueueSize + maxBatchSize;
- Analyze(rate) evaluates throughput/latency/utilization at a rate (req/s);
- Size(targets) inverts the model: binary search for the max rate meeting
  TTFT and ITL targets, TPS handled as lambdaMax*(1 - 0.1) without a search
  (queueanalyzer.go:231-234), final rate = min of the three.

Units: rates are req/s at the public boundary, req/ms internally; latencies
are milliseconds throughout.  No global evaluation state — eval functions are
closures over this instance.
"""

from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass

import numpy as np

from .search import BelowRegion, binary_search
from .statedep import MM1ModelStateDependent

# small disturbance around a value
EPSILON = 0.001
# run this fraction below maximum server throughput for stability
STABILITY_SAFETY_FRACTION = 0.1


class AnalyzerError(RuntimeError):
    """Invalid configuration, request size, target, or model evaluation."""


@dataclass(frozen=True)
class PrefillParms:
    """prefill time = gamma + delta * inputTokens * batchSize (ms)."""

    gamma: float
    delta: float

    def prefill_time(self, avg_input_tokens: int, batch_size: float) -> float:
        if avg_input_tokens == 0:
            return 0.0
        return self.gamma + self.delta * avg_input_tokens * batch_size


@dataclass(frozen=True)
class DecodeParms:
    """decode time = alpha + beta * batchSize (ms)."""

    alpha: float
    beta: float

    def decode_time(self, batch_size: float) -> float:
        return self.alpha + self.beta * batch_size


@dataclass(frozen=True)
class ServiceParms:
    prefill: PrefillParms
    decode: DecodeParms


@dataclass(frozen=True)
class RequestSize:
    avg_input_tokens: int
    avg_output_tokens: int

    def check(self) -> None:
        if self.avg_input_tokens < 0 or self.avg_output_tokens < 1:
            raise AnalyzerError(f"invalid request size {self}")


@dataclass(frozen=True)
class Configuration:
    max_batch_size: int
    max_queue_size: int
    service_parms: ServiceParms

    def check(self) -> None:
        if self.max_batch_size <= 0 or self.max_queue_size < 0 or self.service_parms is None:
            raise AnalyzerError(f"invalid configuration {self}")


@dataclass(frozen=True)
class RateRange:
    """Stable request-rate range in req/s."""

    min: float
    max: float


@dataclass(frozen=True)
class AnalysisMetrics:
    throughput: float  # effective throughput (req/s)
    avg_resp_time: float  # average request latency (ms)
    avg_wait_time: float  # average queueing time (ms)
    avg_num_in_serv: float  # average number of requests in service
    avg_prefill_time: float  # average prefill time (ms)
    avg_token_time: float  # average token decode time (ms)
    max_rate: float  # maximum throughput (req/s)
    rho: float  # utilization


@dataclass(frozen=True)
class TargetPerf:
    target_ttft: float = 0.0  # queueing + prefill (ms); 0 disables
    target_itl: float = 0.0  # inter-token latency (ms); 0 disables
    target_tps: float = 0.0  # token throughput (tok/s); 0 disables
    # allowed probability that TTFT exceeds target_ttft (p95: 0.05); 0 sizes
    # to the mean TTFT; valid values are finite with 0 <= ttft_tail < 1
    ttft_tail: float = 0.0
    # allowed fraction of tokens whose ITL exceeds target_itl (p95: 0.05); 0
    # sizes to the mean ITL; valid values are finite with 0 <= itl_tail < 1
    itl_tail: float = 0.0

    def check(self) -> None:
        if self.target_itl < 0 or self.target_ttft < 0 or self.target_tps < 0:
            raise AnalyzerError(f"invalid target data values {self}")
        if not 0.0 <= self.ttft_tail < 1.0:  # also fails NaN
            raise AnalyzerError(f"invalid TTFT tail probability {self}")
        if not 0.0 <= self.itl_tail < 1.0:  # also fails NaN
            raise AnalyzerError(f"invalid ITL tail fraction {self}")


def _configured_tail(knob: str, what: str, rejected: set) -> float:
    raw = os.environ.get(knob, "").strip()
    if not raw:
        return 0.0
    try:
        percentile = float(raw)
        if percentile < 1.0:  # a fraction, not a percentile: 0.95 is not p0.95
            raise ValueError(raw)
        return percentile_ttft_tail(percentile)
    except ValueError:
        if raw not in rejected:
            rejected.add(raw)
            logging.getLogger("wva_amd.analyzer").warning(
                "%s=%r is not a percentile in [1, 100) such as 95; "
                "sizing to the MEAN %s", knob, raw, what,
            )
        return 0.0


def configured_ttft_tail() -> float:
    """The fleet's TTFT tail probability from ``WVA_TTFT_PERCENTILE`` (read
    per call): ``95`` sizes to the p95 TTFT, ``ttft_tail = 0.05``.  Unset is
    0.0: size to the mean TTFT.  So is a value that is no number in (0, 100)
    (``0.95``, ``100``, ``p95``), with a warning, logged once per value: the
    operator asked for a percentile and is not getting one."""
    return _configured_tail("WVA_TTFT_PERCENTILE", "TTFT", _rejected_percentiles)


def configured_itl_tail() -> float:
    """The fleet's ITL tail fraction from ``WVA_ITL_PERCENTILE`` (read per
    call), with ``WVA_TTFT_PERCENTILE``'s semantics: ``95`` sizes to the p95
    ITL, ``itl_tail = 0.05``; unset is 0.0, the mean ITL, and so is a rejected
    value, with one warning per value."""
    return _configured_tail("WVA_ITL_PERCENTILE", "ITL", _rejected_itl_percentiles)


_rejected_percentiles: set = set()
_rejected_itl_percentiles: set = set()


def percentile_ttft_tail(percentile: float) -> float:
    """``ttft_tail`` of a TTFT percentile in (0, 100); ValueError outside."""
    if not 0.0 < percentile < 100.0:
        raise ValueError(f"TTFT percentile must lie in (0, 100), got {percentile}")
    return (100.0 - percentile) / 100.0


@dataclass(frozen=True)
class TargetRate:
    rate_target_ttft: float  # req/s
    rate_target_itl: float  # req/s
    rate_target_tps: float  # req/s


def effective_concurrency(
    avg_service_time: float,
    service_parms: ServiceParms,
    request_size: RequestSize,
    max_batch_size: int,
) -> float:
    """Effective average number of requests in service: solve
    prefill(n) + (outTokens-1)*decode(n) = avgServiceTime for n,
    clamped to [0, maxBatchSize] (queueanalyzer.go:296-302).
    """
    tokens = float(request_size.avg_output_tokens - 1)
    numerator = avg_service_time - (service_parms.prefill.gamma + service_parms.decode.alpha * tokens)
    denominator = service_parms.prefill.delta * request_size.avg_input_tokens + service_parms.decode.beta * tokens
    if denominator == 0.0:
        # degenerate linear model (e.g. one output token with no prefill
        # slope): any n satisfies the identity up to the constant term
        return float(max_batch_size) if numerator > 0 else 0.0
    n = numerator / denominator
    return min(max(n, 0.0), float(max_batch_size))


def build_service_rates(config: Configuration, request_size: RequestSize) -> np.ndarray:
    """State-dependent service rates mu(n), n = 1..maxBatchSize, in req/ms."""
    parms = config.service_parms
    n = np.arange(1, config.max_batch_size + 1, dtype=np.float64)
    if request_size.avg_input_tokens == 0:
        prefill = np.zeros_like(n)
    else:
        prefill = parms.prefill.gamma + parms.prefill.delta * request_size.avg_input_tokens * n
    num_decode = request_size.avg_output_tokens - 1
    if request_size.avg_input_tokens == 0 and request_size.avg_output_tokens == 1:
        num_decode = 1
    decode = num_decode * (parms.decode.alpha + parms.decode.beta * n)
    return n / (prefill + decode)


class QueueAnalyzer:
    """Analyzer of one inference-server queue for a fixed (model, accelerator,
    request-shape) point.

    ``scv`` (squared coefficient of variation of service time) selects the
    queueing model family: 1.0 (default) is the reference's Markovian
    M/M/1/K contract; any other value applies the Allen-Cunneen wait
    scaling ``(1 + cs^2)/2`` (exact for M/G/1) to every waiting-time
    prediction — inside the Size bisections too, so lambda* and replica
    counts respond.  Opt in fleet-wide with ``WVA_ANALYZER=mg1`` +
    ``WVA_SERVICE_SCV`` (see analyzer/mg1.py for the theory and
    docs/design/mg1-analyzer.md for measured margins)."""

    def __init__(
        self, config: Configuration, request_size: RequestSize, scv: float = 1.0
    ) -> None:
        config.check()
        request_size.check()
        if scv < 0:
            raise AnalyzerError(f"invalid service-time scv {scv}")
        self.max_batch_size = config.max_batch_size
        self.max_queue_size = config.max_queue_size
        self.service_parms = config.service_parms
        self.request_size = request_size
        self.scv = scv
        self._wait_scale = (1.0 + scv) / 2.0

        serv_rate = build_service_rates(config, request_size)
        self.serv_rate = serv_rate
        lambda_min = float(serv_rate[0]) * EPSILON
        lambda_max = float(serv_rate[-1]) * (1.0 - EPSILON)
        self.rate_range = RateRange(min=lambda_min * 1000.0, max=lambda_max * 1000.0)
        occupancy_upper_bound = config.max_queue_size + config.max_batch_size
        self.model = MM1ModelStateDependent(occupancy_upper_bound, serv_rate)

    # -- evaluation ---------------------------------------------------------
    def _solve(self, lam_per_ms: float) -> MM1ModelStateDependent:
        self.model.solve(lam_per_ms, 1.0)
        if not self.model.is_valid:
            raise AnalyzerError(f"invalid model {self.model!r}")
        return self.model

    def _eval_ttft(self, lam_per_ms: float) -> float:
        m = self._solve(lam_per_ms)
        eff_conc = effective_concurrency(
            m.avg_serv_time, self.service_parms, self.request_size, self.max_batch_size
        )
        return m.avg_wait_time * self._wait_scale + self.service_parms.prefill.prefill_time(
            self.request_size.avg_input_tokens, eff_conc
        )

    def _eval_itl(self, lam_per_ms: float) -> float:
        m = self._solve(lam_per_ms)
        eff_conc = effective_concurrency(
            m.avg_serv_time, self.service_parms, self.request_size, self.max_batch_size
        )
        return self.service_parms.decode.decode_time(eff_conc)

    def wait_exceedance(self, request_rate: float, t: float) -> float:
        """P(W > t): the probability that an accepted arrival at
        ``request_rate`` (req/s) waits longer than ``t`` ms for a batch slot.

        The direct definition, and the specification of every native
        implementation (csrc/queue_core.h, "Waiting-time tail"): an accepted
        arrival sees state n with probability p[n] / (1 - p[K]); with n >= N
        ahead of it, it waits for j = n - N + 1 departures at the full-batch
        rate mu_N, an Erlang(j, mu_N) time, so with x = mu_N * t

            P(W > t) = sum_{n=N..K-1} pi_n * sum_{i<j} e^-x x^i / i!.

        ``t <= 0`` gives 1.0, as the TTFT search wants it for a target that
        prefill alone already misses."""
        return self._wait_exceedance(request_rate / 1000.0, t)

    def _wait_exceedance(self, lam_per_ms: float, t: float) -> float:
        m = self._solve(lam_per_ms)
        if not t > 0:
            return 1.0
        N, K = self.max_batch_size, self.model.K
        if K <= N:
            return 0.0  # no queue: nobody waits
        pi = m.p[N:K] / (1.0 - m.p[K])
        x = float(self.serv_rate[-1]) * t
        i = np.arange(K - N, dtype=np.float64)
        log_fact = np.cumsum(np.log(np.maximum(i, 1.0)))
        erlang = np.cumsum(np.exp(i * math.log(x) - x - log_fact))  # [j - 1]: sum over i < j
        return float(np.dot(pi, erlang))

    def ttft_quantile(self, request_rate: float, eps: float) -> float:
        """The TTFT (ms) that an accepted arrival at ``request_rate`` (req/s)
        exceeds with probability ``eps``: ``eps = 0.05`` is the p95 TTFT.

        The inverse of ``wait_exceedance`` and the specification of every
        native implementation (csrc/queue_core.h, "TTFT quantile").  With
        ``p_wait = P(W > 0)``: nobody waits that often when ``p_wait <= eps``,
        and t = 0; otherwise t is the root of ``P(W > t) = eps``, by
        ``binary_search`` on ``[0, t_hi]`` with ``y(0) := p_wait``, where
        ``t_hi = (J + sqrt(2 J l) + l) / mu_N``, ``J`` the queue length and
        ``l = ln(2 / eps)``, holds ``P(W > t_hi) <= eps / 2`` (every
        conditional wait is below Erlang(J, mu_N); Laurent-Massart).  The
        result is ``wait_scale * t + prefill`` at the mean model's effective
        concurrency.  Raises :class:`AnalyzerError` for an ``eps`` outside the
        open (0, 1) and for a rate ``analyze`` rejects."""
        if not 0.0 < eps < 1.0:  # also fails NaN
            raise AnalyzerError(f"invalid TTFT tail probability {eps}")
        if not 0.0 < request_rate <= self.rate_range.max:  # also fails NaN
            raise AnalyzerError(f"invalid request rate {request_rate}")
        lam = request_rate / 1000.0
        m = self._solve(lam)
        eff_conc = effective_concurrency(
            m.avg_serv_time, self.service_parms, self.request_size, self.max_batch_size
        )
        prefill = self.service_parms.prefill.prefill_time(
            self.request_size.avg_input_tokens, eff_conc
        )
        N, K = self.max_batch_size, self.model.K
        p_wait = float(m.p[N:K].sum() / (1.0 - m.p[K]))
        t = 0.0
        if p_wait > eps:
            J, mu_n, l = K - N, float(self.serv_rate[-1]), math.log(2.0 / eps)
            t_hi = (J + math.sqrt(2.0 * J * l) + l) / mu_n
            t, _ = binary_search(
                0.0, t_hi, eps, lambda x: self._wait_exceedance(lam, x) if x > 0 else p_wait
            )
        return self._wait_scale * t + prefill

    def _eval_ttft_tail(self, target_ttft: float):
        """lam -> P(TTFT > target_ttft): the waiting time, stretched by the
        M/G/1 wait scale like the mean, has to fit what prefill leaves."""

        def exceedance(lam_per_ms: float) -> float:
            m = self._solve(lam_per_ms)
            eff_conc = effective_concurrency(
                m.avg_serv_time, self.service_parms, self.request_size, self.max_batch_size
            )
            prefill = self.service_parms.prefill.prefill_time(
                self.request_size.avg_input_tokens, eff_conc
            )
            return self._wait_exceedance(lam_per_ms, (target_ttft - prefill) / self._wait_scale)

        return exceedance

    def itl_exceedance(self, request_rate: float, target_itl: float) -> float:
        """The fraction of tokens emitted at ``request_rate`` (req/s) whose
        inter-token latency exceeds ``target_itl`` ms.

        The direct definition, and the specification of every native
        implementation (csrc/queue_core.h, "Occupancy tail"): a decode step
        with ``b = min(n, N)`` requests in service takes ``decode_time(b)``, and
        state n completes requests at rate mu(n), so tokens are emitted in
        proportion to ``p[n] * mu(n)``:

            y = sum_{n=1..K, decode_time(min(n,N)) > target} p[n] mu(n)
                / sum_{n=1..K} p[n] mu(n)."""
        return self._itl_exceedance(request_rate / 1000.0, target_itl)

    def _itl_exceedance(self, lam_per_ms: float, target_itl: float) -> float:
        m = self._solve(lam_per_ms)
        N, K = self.max_batch_size, self.model.K
        batch = np.minimum(np.arange(1, K + 1), N)
        tokens = m.p[1:] * self.serv_rate[batch - 1]
        decode = self.service_parms.decode
        slow = decode.alpha + decode.beta * batch.astype(np.float64) > target_itl
        return float(tokens[slow].sum() / tokens.sum())

    def itl_quantile(self, request_rate: float, eps: float) -> float:
        """The inter-token latency (ms) that a fraction ``eps`` of the tokens
        emitted at ``request_rate`` (req/s) exceeds: ``eps = 0.05`` is the p95
        ITL.

        The inverse of ``itl_exceedance`` at a fixed rate and the specification
        of every native implementation (csrc/queue_core.h, "ITL quantile").
        With ``S_b`` the share of tokens emitted in decode steps with more than
        b requests in service (``itl_exceedance``'s token weights; 0 for b =
        N), which never grows with b,

            b* = min{b in 1..N : S_b <= eps},   q = decode_time(b*).

        It is stated on the batch count, not on decode times, so ``beta = 0``
        and ``N = 1`` are no special cases.  The service-time cs^2 plays no
        part.  Raises :class:`AnalyzerError` for an ``eps`` outside the open
        (0, 1) and for a rate ``analyze`` rejects."""
        if not 0.0 < eps < 1.0:  # also fails NaN
            raise AnalyzerError(f"invalid ITL tail fraction {eps}")
        if not 0.0 < request_rate <= self.rate_range.max:  # also fails NaN
            raise AnalyzerError(f"invalid request rate {request_rate}")
        m = self._solve(request_rate / 1000.0)
        N, K = self.max_batch_size, self.model.K
        batch = np.minimum(np.arange(1, K + 1), N)
        tokens = m.p[1:] * self.serv_rate[batch - 1]  # [n - 1]: state n
        above = np.cumsum(tokens[::-1])[::-1]  # [b]: the states n > b, summed from the top
        meets = np.flatnonzero(above[1:N] <= eps * above[0])  # [b - 1], b < N
        b = int(meets[0]) + 1 if meets.size else N
        return self.service_parms.decode.decode_time(float(b))

    # -- public API ---------------------------------------------------------
    def analyze(self, request_rate: float) -> AnalysisMetrics:
        """Evaluate performance metrics at a given request rate (req/s)."""
        if request_rate <= 0:
            raise AnalyzerError(f"invalid request rate {request_rate}")
        if request_rate > self.rate_range.max:
            raise AnalyzerError(
                f"rate={request_rate}, max allowed rate={self.rate_range.max}"
            )
        m = self._solve(request_rate / 1000.0)
        avg_num_in_serv = m.avg_num_in_servers
        eff_conc = effective_concurrency(
            m.avg_serv_time, self.service_parms, self.request_size, self.max_batch_size
        )
        prefill_time = self.service_parms.prefill.prefill_time(
            self.request_size.avg_input_tokens, eff_conc
        )
        token_time = self.service_parms.decode.decode_time(eff_conc)
        rho = min(max(avg_num_in_serv / float(self.max_batch_size), 0.0), 1.0)
        corrected_wait = m.avg_wait_time * self._wait_scale
        # scv == 1 keeps the reference's exact Markovian resp time
        # (including its wait>=0 clamp edge case)
        resp = (
            m.avg_resp_time
            if self._wait_scale == 1.0
            else m.avg_serv_time + corrected_wait
        )
        return AnalysisMetrics(
            throughput=m.throughput * 1000.0,
            avg_resp_time=resp,
            avg_wait_time=corrected_wait,
            avg_num_in_serv=avg_num_in_serv,
            avg_prefill_time=prefill_time,
            avg_token_time=token_time,
            max_rate=self.rate_range.max,
            rho=rho,
        )

    def size(self, target_perf: TargetPerf):
        """Max request rates achieving the targets.

        Returns ``(target_rate, metrics, achieved)`` where ``metrics`` is the
        analysis at the min of the three max rates.  Raises
        :class:`AnalyzerError` when a target lies below the reachable region
        (=> no feasible allocation upstream).
        """
        target_perf.check()
        lambda_min = self.rate_range.min / 1000.0
        lambda_max = self.rate_range.max / 1000.0

        lambda_star_ttft = lambda_max
        if target_perf.target_ttft > 0 and target_perf.ttft_tail > 0:
            # percentile target: P(TTFT > target_ttft) against ttft_tail
            lambda_star_ttft, ind = binary_search(
                lambda_min, lambda_max, target_perf.ttft_tail,
                self._eval_ttft_tail(target_perf.target_ttft),
            )
            if ind == BelowRegion:
                raise AnalyzerError(
                    f"failed to calculate lambdaStarTTFT: P(TTFT > {target_perf.target_ttft}) "
                    f"exceeds {target_perf.ttft_tail} on the bounded region {self.rate_range}"
                )
        elif target_perf.target_ttft > 0:
            lambda_star_ttft, ind = binary_search(
                lambda_min, lambda_max, target_perf.target_ttft, self._eval_ttft
            )
            if ind == BelowRegion:
                raise AnalyzerError(
                    f"failed to calculate lambdaStarTTFT: target {target_perf.target_ttft} "
                    f"is below the bounded region {self.rate_range}"
                )

        lambda_star_itl = lambda_max
        if target_perf.target_itl > 0 and target_perf.itl_tail > 0:
            # percentile target: the share of tokens slower than target_itl
            # against itl_tail
            lambda_star_itl, ind = binary_search(
                lambda_min, lambda_max, target_perf.itl_tail,
                lambda lam: self._itl_exceedance(lam, target_perf.target_itl),
            )
            if ind == BelowRegion:
                raise AnalyzerError(
                    f"failed to calculate lambdaStarITL: the share of tokens above "
                    f"{target_perf.target_itl} exceeds {target_perf.itl_tail} on the bounded "
                    f"region {self.rate_range}"
                )
        elif target_perf.target_itl > 0:
            lambda_star_itl, ind = binary_search(
                lambda_min, lambda_max, target_perf.target_itl, self._eval_itl
            )
            if ind == BelowRegion:
                raise AnalyzerError(
                    f"failed to calculate lambdaStarITL: target {target_perf.target_itl} "
                    f"is below the bounded region {self.rate_range}"
                )

        lambda_star_tps = lambda_max
        if target_perf.target_tps > 0:
            lambda_star_tps = lambda_max * (1.0 - STABILITY_SAFETY_FRACTION)

        lam = min(lambda_star_ttft, lambda_star_itl, lambda_star_tps)
        metrics = self.analyze(lam * 1000.0)

        target_rate = TargetRate(
            rate_target_ttft=lambda_star_ttft * 1000.0,
            rate_target_itl=lambda_star_itl * 1000.0,
            rate_target_tps=lambda_star_tps * 1000.0,
        )
        achieved = TargetPerf(
            target_ttft=metrics.avg_wait_time + metrics.avg_prefill_time,
            target_itl=metrics.avg_token_time,
            target_tps=metrics.throughput * self.request_size.avg_output_tokens,
        )
        return target_rate, metrics, achieved
