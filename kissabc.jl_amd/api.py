"""Host-side mirror of the reference's user API for the walker-update path:

    ApproxKernelizedPosterior(prior, cost, scale)      src/types.jl:40-49
    ApproxPosterior(prior, cost, maxcost)              src/types.jl:76-82
    AIS(nparticles)                                    src/KissABC.jl:21-23
    sample(model, AIS(N), Ns; ntransitions, discard_initial, retry_sampling)
    sample(model, AIS(N), MCMCThreads(), Ns, Nc; ...)  src/KissABC.jl:106-173
    smc(prior, cost; kwargs...)                        src/smc.jl:92-206

Everything numerical happens in libkabc_hip.so (gfx950 kernels) behind the C
ABI of include/kabc.h.  This file only marshals arguments and shapes results
(bundle_samples / chainsstack, src/KissABC.jl:82-104).
"""
import collections
import contextlib
import concurrent.futures
import ctypes as C
import math
import time

import numpy as np

from . import _cdefs as cd
from . import _lib
from .costs import DeviceCost
from .distributions import Factored, UnivariateDistribution, as_factored


class Particles:
    """Minimal stand-in for MonteCarloMeasurements.Particles (one parameter's
    samples): the container `bundle_samples` builds (src/KissABC.jl:91)."""

    def __init__(self, particles):
        self.particles = np.asarray(particles)

    def __len__(self):
        return self.particles.shape[0]

    def mean(self):
        return float(np.mean(self.particles))

    def std(self):
        return float(np.std(self.particles, ddof=1))

    def var(self):
        return float(np.var(self.particles, ddof=1))

    def quantile(self, q):
        """numpy.quantile of the samples: a float for a scalar q, an array for a sequence"""
        v = np.quantile(self.particles, q)
        return float(v) if np.ndim(v) == 0 else v

    def isapprox(self, c, nsigma=2.0):
        """MonteCarloMeasurements `p ≈ c`: |mean − c| < nsigma · std."""
        return abs(self.mean() - c) < nsigma * self.std()

    def __array__(self, dtype=None, copy=None):
        return self.particles if dtype is None else self.particles.astype(dtype)

    def __repr__(self):
        return f"{self.mean():.4g} ± {self.std():.2g}"


class PosteriorSummary:
    """Moments of an AIS trace, accumulated on the device instead of the trace (AisEnsemble.summary,
    sample(..., summary=True); include/kabc.h gives the definition, operation by operation):

        n                number of samples, generations x nparticles
        mean, std        per parameter [D]
        cov              [D][D] ("full"), or the variances [D] ("diag", beyond KABC_MAX_DIM parameters)
        min, max         per parameter
        pivot, sum1, sum2   the raw sums behind them: sums of (x - pivot) and of its products

    With summary_begin(autocorr=...) / sample(..., autocorr=...), else None:

        tau, ess         integrated autocorrelation time in generations and n / tau, per parameter [D]
        mcse             Monte Carlo standard error of the mean: std * sqrt(tau / n)
        acf, acov        autocorrelation and autocovariance [D][nlags] at lags 0 ... nlags - 1
        window           Sokal's automatic window (c = 5) per parameter; tau_converged: it lies inside maxlag
        maxlag           the largest lag kept

    With summary_begin(derived=d) / sample(..., derived=d), else None:

        derived          a PosteriorSummary of its own over d's G quantities of every trace row, with every field
                         and method listed here and `.names`, d's labels (`names` is None on the parameters' own)

    With summary_begin(hist=...) / sample(..., hist=...), else None (and quantile() raises):

        hist             marginal histogram per parameter [D][nbins], uint64 counts
        edges            its bin edges [D][nbins + 1]: lo + j * (hi - lo) / nbins, the last one hi itself
        underflow, overflow   samples below lo / not below hi (a NaN counts as overflow), per parameter [D]
        quantile(q), median, interval(level)   read from the counts by kabc_hist_quantile's rule
                         (include/kabc.h): exact at q = 0 and 1 (min and max), within one bin width of the
                         sample's order statistic where that lies inside [lo, hi)

    On a batch handle every array has a leading chain axis and chain(c) gives chain c's own summary."""

    def __init__(self, n, mean, cov, min, max, pivot=None, sum1=None, sum2=None, diag=False, autocorr=None,
                 hist=None):
        self.n, self.mean, self.cov, self.min, self.max = int(n), mean, cov, min, max
        self.pivot, self.sum1, self.sum2, self.diag = pivot, sum1, sum2, bool(diag)
        # autocorr: dict of tau, ess, acf, acov, window, tau_converged, maxlag (and the raw lagsum, first, last)
        self.autocorr = autocorr
        for f in self.AUTOCORR_FIELDS:
            setattr(self, f, None if autocorr is None else autocorr.get(f))
        # hist: dict of counts [...][D][nbins + 2] (uint64: underflow, the bins, overflow), lo, hi [...][D]
        self.histogram = hist
        # derived: the PosteriorSummary over a Derived's G quantities (summary_begin(derived=...)), its labels
        # in its `.names`; None on a summary without one
        self.derived = None
        self.names = None

    AUTOCORR_FIELDS = ("tau", "ess", "acf", "acov", "window", "tau_converged", "maxlag", "lagsum", "first", "last")

    @property
    def hist(self):
        return None if self.histogram is None else self.histogram["counts"][..., 1:-1]

    @property
    def underflow(self):
        return None if self.histogram is None else self.histogram["counts"][..., 0]

    @property
    def overflow(self):
        return None if self.histogram is None else self.histogram["counts"][..., -1]

    @property
    def nbins(self):
        return None if self.histogram is None else self.histogram["counts"].shape[-1] - 2

    @property
    def edges(self):
        if self.histogram is None:
            return None
        lo, hi, B = self.histogram["lo"][..., None], self.histogram["hi"][..., None], self.nbins
        e = lo + np.arange(B + 1) * ((hi - lo) / B)
        e[..., -1] = hi[..., 0]
        return e

    def quantile(self, q):
        """The q-quantile (q in [0, 1], a scalar or a sequence) of every parameter from its histogram:
        [D] for a scalar q, else [D][len(q)]; a leading chain axis on a batch summary."""
        if self.histogram is None:
            raise ValueError(self.NO_HIST)
        qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        if qs.ndim != 1:
            raise ValueError("quantile: q must be a scalar or a sequence")
        counts = np.ascontiguousarray(self.histogram["counts"], dtype=np.uint64)
        B = counts.shape[-1] - 2
        lo, hi = self.histogram["lo"], self.histogram["hi"]
        out = np.empty(lo.shape + (qs.size,))
        lib = _lib.load()
        for idx in np.ndindex(*lo.shape):
            c, o = counts[idx], out[idx]
            _lib.check(lib.kabc_hist_quantile(c.ctypes.data_as(C.POINTER(C.c_uint64)), B, float(lo[idx]),
                                              float(hi[idx]), float(self.min[idx]), float(self.max[idx]),
                                              qs.ctypes.data_as(cd.c_double_p), qs.size,
                                              o.ctypes.data_as(cd.c_double_p)))
        return out[..., 0] if np.ndim(q) == 0 else out

    NO_HIST = "this summary carries no histogram: open it with summary_begin(hist=...) / sample(..., hist=...)"

    @property
    def median(self):
        return None if self.histogram is None else self.quantile(0.5)

    def interval(self, level=0.95):
        """The central credible interval: the quantiles at (1 - level) / 2 and (1 + level) / 2, [D][2]"""
        return self.quantile([(1.0 - level) / 2.0, (1.0 + level) / 2.0])

    @property
    def mcse(self):
        return None if self.tau is None else self.std * np.sqrt(self.tau / self.n)

    @property
    def var(self):
        return self.cov if self.diag else np.diagonal(self.cov, axis1=-2, axis2=-1)

    @property
    def std(self):
        return np.sqrt(self.var)

    @property
    def nchains(self):
        """chains on the leading axis, None for a single summary"""
        return self.mean.shape[0] if self.mean.ndim == 2 else None

    def chain(self, c):
        if self.nchains is None:
            raise ValueError("this summary holds one chain")
        pick = lambda a: None if a is None else a[c]   # noqa: E731
        ac = self.autocorr
        if ac is not None:
            ac = {f: (v if f == "maxlag" else pick(v)) for f, v in ac.items()}
        hs = self.histogram
        if hs is not None:
            hs = {f: pick(v) for f, v in hs.items()}
        out = PosteriorSummary(self.n, self.mean[c], self.cov[c], self.min[c], self.max[c], pick(self.pivot),
                               pick(self.sum1), pick(self.sum2), self.diag, ac, hs)
        out.names = self.names
        if self.derived is not None:
            out.derived = self.derived.chain(c)
        return out

    def isapprox(self, c, nsigma=2.0):
        """Particles.isapprox per parameter: |mean - c| < nsigma * std, an array of bool"""
        return np.abs(self.mean - np.asarray(c, dtype=np.float64)) < nsigma * self.std

    def __repr__(self):
        if self.nchains is not None:
            return "[" + ",\n ".join(repr(self.chain(c)) for c in range(self.nchains)) + "]"
        return "[" + ", ".join(f"{m:.4g} ± {sd:.2g}" for m, sd in zip(self.mean, self.std)) + "]"


class ChainSummaries(list):
    """sample(model, AIS(N), MCMCThreads(), Ns, Nc, summary=True): one PosteriorSummary per chain, `.pooled`
    (the chains merged on the host, in chain order, from their n, mean and cov) and `.rhat` (Gelman-Rubin's
    potential scale reduction per parameter, from the per-chain means and variances).  With `hist`, `.pooled`
    carries the sum of the chains' counts where every chain has the same bins bit for bit -- a range the
    caller gave, hist=(lo, hi); the automatic range is each chain's own, and `.pooled.hist` is then None."""

    def __init__(self, chains):
        super().__init__(chains)
        self.pooled = _pool_summaries(self)
        self.rhat = _rhat(self)
        # with autocorr: the chains are independent, so their effective sample sizes add (pooled.tau stays None)
        self.ess = None if self[0].ess is None else np.sum(np.stack([c.ess for c in self]), axis=0)
        # with derived: the chains' derived summaries pooled by this same code -- `.derived` is their
        # ChainSummaries (its .pooled, .rhat and .ess), and `.pooled.derived` its pooled summary
        self.derived = None
        if all(c.derived is not None for c in self):
            self.derived = ChainSummaries(c.derived for c in self)
            self.derived.pooled.names = self[0].derived.names
            self.pooled.derived = self.derived.pooled


def _pool_summaries(chains):
    """the pairwise update of Chan, Golub & LeVeque, chain after chain: n, mean and the centred sum of
    products M2 = cov * (n - 1)"""
    c0 = chains[0]
    n, mean, m2 = c0.n, np.array(c0.mean, dtype=np.float64), np.array(c0.cov, dtype=np.float64) * (c0.n - 1)
    mn, mx = np.array(c0.min), np.array(c0.max)
    for c in chains[1:]:
        tot = n + c.n
        delta = c.mean - mean
        cross = delta * delta if c0.diag else np.outer(delta, delta)
        m2 = m2 + c.cov * (c.n - 1) + cross * (n * c.n / tot)
        mean = mean + delta * (c.n / tot)
        n = tot
        mn, mx = np.minimum(mn, c.min), np.maximum(mx, c.max)
    pooled = PosteriorSummary(n, mean, m2 / (n - 1), mn, mx, diag=c0.diag, hist=_pool_histograms(chains))
    if c0.histogram is not None and pooled.histogram is None:
        pooled.NO_HIST = ("the chains' histograms have different ranges (the automatic range is each chain's own): "
                          "pass hist=(lo, hi) to pool their counts")
    return pooled


def _pool_histograms(chains):
    """the sum of the chains' counts where all have the same lo, hi and nbins bit for bit, else None"""
    hs = [c.histogram for c in chains]
    if any(h is None for h in hs):
        return None
    h0 = hs[0]
    same = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()   # noqa: E731
    for h in hs[1:]:
        if h["counts"].shape != h0["counts"].shape or not same(h["lo"], h0["lo"]) or not same(h["hi"], h0["hi"]):
            return None
    return {"counts": np.sum(np.stack([h["counts"] for h in hs]), axis=0, dtype=np.uint64),
            "lo": np.array(h0["lo"]), "hi": np.array(h0["hi"])}


def _rhat(chains):
    """sqrt(((n - 1) / n * W + B / n) / W): W the mean of the chains' variances, B / n the variance of their
    means; NaN with one chain"""
    n = chains[0].n
    means = np.stack([c.mean for c in chains])
    W = np.mean(np.stack([c.var for c in chains]), axis=0)
    if len(chains) < 2:
        return np.full(means.shape[1], np.nan)
    b_over_n = np.var(means, axis=0, ddof=1)
    return np.sqrt(((n - 1) / n * W + b_over_n) / W)


class _ApproxModel:
    posterior = 0

    def __init__(self, prior, cost, eps):
        self.prior = as_factored(prior)
        self.scalar = isinstance(prior, UnivariateDistribution)
        if not isinstance(cost, DeviceCost):
            raise TypeError(
                "on the MI355X path `cost` must be a DeviceCost (kissabc_jl_amd.costs.*): a host "
                "closure cannot be called from a gfx950 kernel")
        self.cost = cost
        self.eps = float(eps)

    def __len__(self):  # length(density) = length(prior), src/types.jl:37
        return len(self.prior)

    def to_c(self):
        m = cd.Model()
        self._prior_c = self.prior.to_c()
        m.prior = C.cast(self._prior_c, C.POINTER(cd.Prior))
        m.D = len(self.prior)
        m.posterior = self.posterior
        m.eps = self.eps
        m.cost = self.cost.to_c()
        return m


class ApproxKernelizedPosterior(_ApproxModel):
    """Gaussian-kernel ABC density; `scale` = target_average_cost (src/types.jl:130-139)."""
    posterior = cd.POSTERIOR_KERNELIZED

    @property
    def scale(self):
        return self.eps


class ApproxPosterior(_ApproxModel):
    """Hard-threshold ABC density; `maxcost` (src/types.jl:140-149)."""
    posterior = cd.POSTERIOR_THRESHOLD

    @property
    def maxcost(self):
        return self.eps


class CommonLogDensity(_ApproxModel):
    """CommonLogDensity(nparameters, sample_init, lπ) -- src/types.jl:105-128, 151-161:
    classical MCMC on a log-density.  On the device path `lπ` is a DeviceCost that
    RETURNS THE LOG-DENSITY (built-in or costs.UserCost) and `sample_init` is a
    Factored / univariate distribution the initial walkers are drawn from -- or
    `InitFromSnippet(nparameters)`: the reference takes an arbitrary `rng -> sample` closure,
    here the log-density's C snippet may bring its own (`#define KABC_USER_SAMPLE_INIT 1` +
    `kabc_user_sample_init(x, D, params, data, ndata, rng)`, include/kabc_costs.h)."""
    posterior = cd.POSTERIOR_COMMON

    def __init__(self, nparameters, sample_init, lpi):
        super().__init__(sample_init, lpi, 1.0)
        if len(self.prior) != int(nparameters):
            raise ValueError("nparameters must equal the length of sample_init")

    @property
    def lπ(self):
        return self.cost


def compile_model(model_or_prior, cost=None, families=0):
    """Compile kernels specialised for ONE model (kabc_compile_model, include/kabc.h): the prior
    tuple's families and parameters become compile-time constants of a run-time compiled
    translation unit.  compile_model(model) for an ApproxKernelizedPosterior / ApproxPosterior,
    compile_model(prior, cost) for smc / ABCDE / pfilter; `families`: bit mask of
    cd.FAMILY_AIS / _SMC / _ABCDE / _PFILTER (0 = AIS + smc).  Afterwards sample / smc / ... on
    the same prior components and cost use the specialised kernels; results keep their bits.
    Returns the registration's handle (0: the model is left to the prebuilt kernels)."""
    if cost is None:
        m = model_or_prior.to_c()
        keep = model_or_prior
    else:
        keep = _ApproxModel(model_or_prior, cost, 1.0)
        m = keep.to_c()
    h = C.c_int32()
    _lib.check(_lib.load().kabc_compile_model(C.byref(m), int(families), C.byref(h)))
    del keep
    return int(h.value)


def set_specialize(mode):
    """kabc_set_specialize: "env" (KABC_SPECIALIZE decides), "off" (never specialise, never start the
    compiler worker process), "blocking" (compile at first sight), "background" (the worker)."""
    m = {"env": -1, "off": 0, "blocking": 1, "background": 2}[mode]
    _lib.check(_lib.load().kabc_set_specialize(m))


class AIS:
    """AIS(nparticles) -- src/KissABC.jl:21-23"""

    def __init__(self, nparticles):
        self.nparticles = int(nparticles)


class MCMCThreads:
    """Tag for independent chains (AbstractMCMC.MCMCThreads, re-exported at
    src/KissABC.jl:9,175).  On this path chains are independent ensembles with
    distinct seeds advanced TOGETHER: chain is a grid dimension of every launch."""


AUTOCORR_DEFAULT_LAG = 64


def _autocorr_maxlag(autocorr, who):
    """autocorr: None / False (off: 0), True (AUTOCORR_DEFAULT_LAG) or an int in 1 ... KABC_AUTOCORR_MAX_LAG"""
    if autocorr is None or autocorr is False:
        return 0
    if autocorr is True:
        return AUTOCORR_DEFAULT_LAG
    if isinstance(autocorr, (int, np.integer)) and 1 <= int(autocorr) <= cd.KABC_AUTOCORR_MAX_LAG:
        return int(autocorr)
    raise ValueError(f"{who}: autocorr must be None, a bool or a maximum lag in 1 ... "
                     f"{cd.KABC_AUTOCORR_MAX_LAG}, not {autocorr!r}")


HIST_DEFAULT_BINS = 128


def _hist_spec(hist, who):
    """hist: None / False (off: None), True (HIST_DEFAULT_BINS bins, automatic range), an int (that many bins,
    automatic range), (lo, hi) or (lo, hi, nbins)  ->  (nbins, lo, hi); lo and hi are None for the automatic
    range, else float64 arrays still to be broadcast to the handle's [chain][D] (_hist_range)"""
    if hist is None or hist is False:
        return None
    bad = ValueError(f"{who}: hist must be None, a bool, a number of bins in 1 ... {cd.KABC_HIST_MAX_BINS}, "
                     f"(lo, hi) or (lo, hi, nbins), not {hist!r}")
    is_bins = lambda b: (isinstance(b, (int, np.integer)) and not isinstance(b, bool)   # noqa: E731
                         and 1 <= int(b) <= cd.KABC_HIST_MAX_BINS)
    if hist is True:
        return HIST_DEFAULT_BINS, None, None
    if isinstance(hist, (int, np.integer)):
        if not is_bins(hist):
            raise bad
        return int(hist), None, None
    if not isinstance(hist, (tuple, list)) or len(hist) not in (2, 3):
        raise bad
    nbins = HIST_DEFAULT_BINS
    if len(hist) == 3:
        if not is_bins(hist[2]):
            raise bad
        nbins = int(hist[2])
    try:
        lo, hi = (np.asarray(v, dtype=np.float64) for v in hist[:2])
    except (TypeError, ValueError):
        raise bad from None
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError(f"{who}: hist: lo and hi must be finite")
    return nbins, lo, hi


def _hist_range(lo, hi, nchains, D, who):
    """lo, hi (scalars, [D] or [chain][D]) as C-contiguous [nchains][D] with lo < hi everywhere"""
    out = []
    for name, v in (("lo", lo), ("hi", hi)):
        if v.shape not in ((), (D,), (nchains, D)):
            raise ValueError(f"{who}: hist: {name} must be a scalar, [D] = [{D}] or [chain][D] = [{nchains}][{D}], "
                             f"not of shape {list(v.shape)}")
        out.append(np.ascontiguousarray(np.broadcast_to(v, (nchains, D))))
    if not np.all(out[0] < out[1]):
        c, k = np.argwhere(~(out[0] < out[1]))[0]
        raise ValueError(f"{who}: hist: chain {c}, parameter {k}: lo = {out[0][c, k]!r} is not below "
                         f"hi = {out[1][c, k]!r}")
    return out


def _derived_check(derived, who, summary=True, sharded=False):
    """the refusals of `derived=` that need no library"""
    if derived is None:
        return
    from .derived import Derived
    if not isinstance(derived, Derived):
        raise TypeError(f"{who}: derived must be a Derived, not {type(derived).__name__}")
    if not summary:
        raise ValueError(f"{who}: derived quantities are accumulated by the device summary; derived= needs "
                         "summary=True (on a returned trace, call derived(trace) instead)")
    if sharded:
        raise ValueError(f"{who}: a sharded ensemble has no streamed trace, and so no summary of one: derived= "
                         "needs a single-process ensemble")


def _hist_auto_range(x):
    """the automatic range from the walkers x [...][N][D]: with mn, mx over the walkers and s = mx - mn,
    lo = mn - s and hi = mx + s; a parameter on which all walkers agree (s == 0) gets mn - 0.5, mx + 0.5"""
    mn, mx = np.min(x, axis=-2), np.max(x, axis=-2)
    s = mx - mn
    flat = s == 0
    return np.where(flat, mn - 0.5, mn - s), np.where(flat, mx + 0.5, mx + s)


class AisEnsemble:
    """kabc_ais_t: the device-resident AISState (src/KissABC.jl:25-33)."""

    def __init__(self, model, nparticles, seed=0, ctx=None, sharded=None, comm=None, seeds=None, costs=None):
        """`seeds` (a sequence) makes a BATCH handle: len(seeds) independent ensembles of
        `nparticles` walkers, chain = a grid dimension of every launch (kabc_ais_create_batch);
        state / trace arrays gain a leading chain axis.  `costs` (a sequence of DeviceCosts, one per
        chain, with model.cost's id and params / data lengths) fits the model to one dataset per
        chain: chain c runs on model with its cost replaced by costs[c] (kabc_ais_create_batch_costs)."""
        if costs is not None:
            if seeds is None:
                raise ValueError("AisEnsemble: costs needs seeds (one per chain)")
            costs = list(costs)
            if not all(isinstance(c, DeviceCost) for c in costs):
                raise TypeError("AisEnsemble: costs must be DeviceCosts")
            if len(costs) != len(seeds):
                raise ValueError(f"AisEnsemble: {len(costs)} costs for {len(seeds)} seeds")
        self.model = model
        self.comm = comm
        self._is_sharded = comm is not None or (sharded is not None and sharded[1] > 1)
        self.nchains = 1 if seeds is None else len(seeds)
        self.batched = seeds is not None
        self.ctx = comm.ctx if comm is not None else (ctx or _lib.default_context())
        self.N = int(nparticles)
        self.D = len(model)
        self._cmodel = model.to_c()
        self._h = C.c_void_p()
        lib = _lib.load()
        if seeds is not None and costs is not None:
            arr = (C.c_uint64 * len(seeds))(*[int(v) & (2 ** 64 - 1) for v in seeds])
            ccs = (cd.Cost * len(costs))(*[c.to_c() for c in costs])   # (copied by the library)
            _lib.check(lib.kabc_ais_create_batch_costs(self.ctx.handle, C.byref(self._cmodel), self.N,
                                                       len(seeds), arr, ccs, C.byref(self._h)))
        elif seeds is not None:
            arr = (C.c_uint64 * len(seeds))(*[int(v) & (2 ** 64 - 1) for v in seeds])
            _lib.check(lib.kabc_ais_create_batch(self.ctx.handle, C.byref(self._cmodel), self.N,
                                                 len(seeds), arr, C.byref(self._h)))
        elif comm is not None:
            # walker-sharded over the communicator's ranks; the library owns the exchange
            _lib.check(lib.kabc_ais_create_dist(comm.handle, C.byref(self._cmodel), self.N,
                                                int(seed), C.byref(self._h)))
        elif sharded is None:
            _lib.check(lib.kabc_ais_create(self.ctx.handle, C.byref(self._cmodel), self.N,
                                           int(seed), C.byref(self._h)))
        else:
            rank, world, p0, p1 = sharded
            _lib.check(lib.kabc_ais_create_sharded(self.ctx.handle, C.byref(self._cmodel), self.N,
                                                   rank, world, int(seed), C.c_void_p(p0),
                                                   C.c_void_p(p1), C.byref(self._h)))
        self.owned = (lib.kabc_ais_owned(self._h, 0), lib.kabc_ais_owned(self._h, 1))

    # step(rng, model, spl; retry_sampling) -- src/KissABC.jl:35-64
    def init(self, retry_sampling=100):
        _lib.check(_lib.load().kabc_ais_init(self._h, int(retry_sampling)))
        return self

    # step(rng, model, spl, state; ntransitions) x N x ngenerations -- src/KissABC.jl:66-80
    def advance(self, ngenerations, ntransitions=1, collect=False, out=None, summary=False):
        """`collect=True` returns the sample trace [generation][walker][D]
        ([generation][chain][walker][D] for a batch handle); `out` may supply its buffer
        (C-contiguous float64, e.g. from _lib.pinned_empty).  `summary=True` folds the trace into the
        summary opened with summary_begin() on the device instead (kabc_ais_advance_summary): nothing is
        returned, summary() reads the moments; it excludes `collect` and `out`."""
        lib = _lib.load()
        if summary:
            if collect or out is not None:
                raise ValueError("advance: summary=True consumes the trace on the device; it excludes collect / out")
            st = cd.Stats()
            with self.ctx.interruptible():
                status = lib.kabc_ais_advance_summary(self._h, int(ngenerations), int(ntransitions), C.byref(st))
                self.last_stats = {"proposals": st.proposals, "cost_evals": st.cost_evals,
                                   "accepted": st.accepted}
                _lib.check(status)
            return None
        ptr = None
        if collect or out is not None:
            shape = ((int(ngenerations), self.nchains, self.N, self.D) if self.batched
                     else (int(ngenerations), self.N, self.D))
            if out is None:
                out = _lib.pinned_empty(shape)
            if out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous float64 array of shape {shape}")
            ptr = out.ctypes.data_as(cd.c_double_p)
        st = cd.Stats()
        # Ctrl-C / Context.cancel(): the call stops at a generation boundary and raises (the handle
        # then holds the state after the generations it completed; include/kabc.h)
        with (self.ctx.interruptible() if self.comm is None else contextlib.nullcontext()):
            status = lib.kabc_ais_advance(self._h, int(ngenerations), int(ntransitions), ptr,
                                          C.byref(st))
            self.last_stats = {"proposals": st.proposals, "cost_evals": st.cost_evals,
                               "accepted": st.accepted}
            _lib.check(status)
        return out

    COV_MODES = {None: cd.SUMMARY_AUTO, "full": cd.SUMMARY_FULL, "diag": cd.SUMMARY_DIAG}

    def summary_begin(self, cov=None, autocorr=None, hist=None, derived=None):
        """Opens (or starts over) the posterior summary of this handle: advance(..., summary=True) then
        accumulates, summary() reads.  cov: "full" (the covariance matrix, up to KABC_MAX_DIM parameters),
        "diag" (the variances, any length(prior)), None (full where it exists, else diag).  autocorr: True
        (maxlag = 64) or a maximum lag adds the lagged products on the device (kabc_ais_autocorr_begin):
        summary() then reports tau, ess and mcse per parameter.

        hist adds a marginal histogram per parameter, counted on the device (kabc_ais_hist_begin): summary()
        then reports hist, edges, underflow, overflow, quantile(q), median and interval(level).  True: 128
        bins over the automatic range; an int: that many bins (up to KABC_HIST_MAX_BINS); (lo, hi) or
        (lo, hi, nbins): the range [lo, hi), each a scalar, [D] or [chain][D].  The automatic range is taken
        per chain and parameter from the walkers as they stand now: with mn, mx over them and s = mx - mn,
        lo = mn - s and hi = mx + s (mn - 0.5, mx + 0.5 where s == 0).  It is a convention, not a guarantee:
        a chain that has not yet spread, or drifts, leaves it, and `underflow` / `overflow` report how many
        samples it missed.  A discrete parameter wants an explicit integer-aligned range, one bin per value:
        (-0.5, K + 0.5, K + 1) for values 0 ... K.

        derived (a Derived) adds a second set of accumulators over its G quantities of every trace row, mapped
        on the device (kabc_ais_derived_begin): summary().derived is then a PosteriorSummary over them, with
        `.names`.  autocorr and hist (its number of bins) apply to both sets; the derived histograms range over
        derived.hist_range, else over the automatic convention applied to derived(walkers as they stand now).
        "full" covariance up to KABC_MAX_DIM derived values, variances beyond."""
        if cov not in self.COV_MODES:
            raise ValueError(f'summary_begin: cov must be "full", "diag" or None, not {cov!r}')
        maxlag = _autocorr_maxlag(autocorr, "summary_begin")
        spec = _hist_spec(hist, "summary_begin")
        if spec is not None and spec[1] is not None:
            spec = (spec[0], *_hist_range(spec[1], spec[2], self.nchains, self.D, "summary_begin"))
        _derived_check(derived, "summary_begin", sharded=self._is_sharded)
        _lib.check(_lib.load().kabc_ais_summary_begin(self._h, self.COV_MODES[cov]))
        self._summary_diag = cov == "diag" or (cov is None and self.D > cd.KABC_MAX_DIM)
        self._summary_maxlag = 0
        self._summary_hist = 0
        self._summary_derived = None
        if derived is not None:
            # the second set: autocorr and hist (its bin count) apply to it too; its range is derived.hist_range,
            # else the automatic convention applied to derived(walkers as they stand now), per chain
            d, nb, lo, hi = derived, 0, None, None
            if spec is not None:
                nb = spec[0]
                if d.hist_range is not None:
                    lo, hi = (np.ascontiguousarray(np.broadcast_to(v, (self.nchains, d.G))) for v in d.hist_range)
                else:
                    g = d(self.state()[0], ctx=self.ctx)
                    lo, hi = (np.ascontiguousarray(v.reshape(self.nchains, d.G)) for v in _hist_auto_range(g))
            ptr = lambda v: None if v is None else v.ctypes.data_as(cd.c_double_p)   # noqa: E731
            _lib.check(_lib.load().kabc_ais_derived_begin(self._h, d.id, d.G, d._params_ptr(), d.params.size,
                                                          cd.SUMMARY_AUTO, maxlag, nb, ptr(lo), ptr(hi)))
            self._summary_derived = d
        if maxlag:
            _lib.check(_lib.load().kabc_ais_autocorr_begin(self._h, maxlag))
            self._summary_maxlag = maxlag
        if spec is not None:
            nbins, lo, hi = spec
            if lo is None:
                x = self.state()[0]
                lo, hi = (np.ascontiguousarray(v.reshape(self.nchains, self.D)) for v in _hist_auto_range(x))
            _lib.check(_lib.load().kabc_ais_hist_begin(self._h, nbins, lo.ctypes.data_as(cd.c_double_p),
                                                       hi.ctypes.data_as(cd.c_double_p)))
            self._summary_hist = nbins
        return self

    def summary(self):
        """The PosteriorSummary of the generations advanced with summary=True since summary_begin(); with
        summary_begin(derived=d) its `.derived` is the PosteriorSummary of d's G quantities."""
        out = self._read_set(self.D, getattr(self, "_summary_diag", False), getattr(self, "_summary_maxlag", 0),
                             getattr(self, "_summary_hist", 0), "kabc_ais_summary_get", "kabc_ais_autocorr_get",
                             "kabc_ais_hist_get")
        d = getattr(self, "_summary_derived", None)
        if d is not None:
            out.derived = self._read_set(d.G, d.G > cd.KABC_MAX_DIM, self._summary_maxlag, self._summary_hist,
                                         "kabc_ais_derived_summary_get", "kabc_ais_derived_autocorr_get",
                                         "kabc_ais_derived_hist_get")
            out.derived.names = d.names
        return out

    def _read_set(self, D, diag, maxlag, nbins, get, get_autocorr, get_hist):
        """one set of the open summary (the parameters' or the derived values') through its three getters"""
        lib = _lib.load()
        lead = (self.nchains,) if self.batched else ()
        vec = lambda: np.empty(lead + (D,))                              # noqa: E731
        mat = lambda: np.empty(lead + ((D,) if diag else (D, D)))         # noqa: E731
        n = C.c_int64()
        pivot, sum1, mean, mn, mx, sum2, cov = vec(), vec(), vec(), vec(), vec(), mat(), mat()
        p = lambda a: a.ctypes.data_as(cd.c_double_p)                             # noqa: E731
        _lib.check(getattr(lib, get)(self._h, C.byref(n), p(pivot), p(sum1), p(sum2), p(mean), p(cov), p(mn), p(mx)))
        return PosteriorSummary(n.value, mean, cov, mn, mx, pivot, sum1, sum2, diag,
                                self._autocorr(lead, D, maxlag, getattr(lib, get_autocorr)),
                                self._histogram(lead, D, nbins, getattr(lib, get_hist)))

    def _histogram(self, lead, D, B, get):
        """kabc_ais_hist_get of the open summary as PosteriorSummary's dict, None without hist"""
        if not B:
            return None
        nb = C.c_int32()
        counts = np.zeros(lead + (D, B + 2), dtype=np.uint64)
        lo, hi = np.empty(lead + (D,)), np.empty(lead + (D,))
        _lib.check(get(self._h, C.byref(nb), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                       lo.ctypes.data_as(cd.c_double_p), hi.ctypes.data_as(cd.c_double_p)))
        assert nb.value == B, (nb.value, B)
        return {"counts": counts, "lo": lo, "hi": hi}

    def _autocorr(self, lead, D, L, get):
        """kabc_ais_autocorr_get of the open summary as PosteriorSummary's dict, None without autocorr"""
        if not L:
            return None
        nl = C.c_int32()
        lagsum, acov, rho = (np.full(lead + (D, L + 1), np.nan) for _ in range(3))
        first, last = (np.full(lead + (L, D), np.nan) for _ in range(2))
        tau, ess = np.empty(lead + (D,)), np.empty(lead + (D,))
        window, conv = np.zeros(lead + (D,), dtype=np.int32), np.zeros(lead + (D,), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(cd.c_double_p)                             # noqa: E731
        pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                     # noqa: E731
        _lib.check(get(self._h, C.byref(nl), p(lagsum), p(first), p(last), p(acov), p(rho), p(tau), p(ess),
                       pi(window), pi(conv)))
        nl = nl.value
        nw = min(L, nl)                                      # rows of the two windows: min(maxlag, G)
        return {"tau": tau, "ess": ess, "acf": rho[..., :nl], "acov": acov[..., :nl], "window": window,
                "tau_converged": conv.astype(bool), "maxlag": L, "lagsum": lagsum[..., :nl],
                "first": first[..., :nw, :], "last": last[..., :nw, :]}

    def summary_end(self):
        _lib.check(_lib.load().kabc_ais_summary_end(self._h))

    def half_generation(self, half, ntransitions, trace_ptr=None):
        _lib.check(_lib.load().kabc_ais_half_generation(
            self._h, int(half), int(ntransitions), C.c_void_p(trace_ptr) if trace_ptr else None))

    def end_generation(self, ntransitions):
        _lib.check(_lib.load().kabc_ais_end_generation(self._h, int(ntransitions)))

    def state(self):
        n = self.owned[0] + self.owned[1]
        lead = (self.nchains,) if self.batched else ()
        x = np.empty(lead + (n, self.D))
        lp = np.empty(lead + (n,))
        ll = np.empty(lead + (n,))
        t = C.c_uint64()
        _lib.check(_lib.load().kabc_ais_get_state(
            self._h, x.ctypes.data_as(cd.c_double_p), lp.ctypes.data_as(cd.c_double_p),
            ll.ctypes.data_as(cd.c_double_p), C.byref(t)))
        return x, lp, ll, t.value

    def set_state(self, x, lp, ll, t=0):
        x = np.ascontiguousarray(x, dtype=np.float64)
        lp = np.ascontiguousarray(lp, dtype=np.float64)
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        _lib.check(_lib.load().kabc_ais_set_state(
            self._h, x.ctypes.data_as(cd.c_double_p), lp.ctypes.data_as(cd.c_double_p),
            ll.ctypes.data_as(cd.c_double_p), int(t)))

    def segments(self, half):
        """[(first global row of the half, rows), ...]: the owned row ranges of `half` in the
        order state() / get_debug() lay the owned rows out (kabc_ais_owned_segments; one range
        unless the handle is sharded with more than one exchange chunk)."""
        cap = cd.KABC_MAX_EXCHANGE_CHUNKS
        first, count = (C.c_int64 * cap)(), (C.c_int64 * cap)()
        n = _lib.load().kabc_ais_owned_segments(self._h, int(half), first, count, cap)
        return [(first[i], count[i]) for i in range(n)]

    def stats(self):
        st = cd.Stats()
        _lib.check(_lib.load().kabc_ais_get_stats(self._h, C.byref(st)))
        return {"proposals": st.proposals, "cost_evals": st.cost_evals, "accepted": st.accepted}

    SPEC_STATES = ("none", "pending", "active", "failed")   # KABC_SPEC_* of include/kabc.h

    def spec_state(self):
        """(state, launches_before_switch): which kernels the half-generation launches run on --
        the prebuilt ones ("none" / "pending" / "failed") or the model's own ("active", the default
        non-blocking specialisation of include/kabc.h); launches that ran before the switch, -1."""
        st, n = C.c_int32(0), C.c_int64(-1)
        _lib.check(_lib.load().kabc_ais_spec_state(self._h, C.byref(st), C.byref(n)))
        return self.SPEC_STATES[st.value], n.value

    @property
    def driver(self):
        """"small": kabc_ais_advance runs every generation of a call in one launch of one workgroup
        per chain (csrc/ais_small_kernel.hpp; beyond KABC_MAX_DIM parameters csrc/ais_dyn_small_kernel.hpp);
        "halves": one launch per half-generation."""
        return "small" if _lib.load().kabc_ais_driver(self._h) else "halves"

    def ensemble(self):
        """[N][D] unrounded positions of ALL walkers in walker-id order (for a sharded
        handle: this rank's copy after the last all-gather)."""
        x = np.empty(((self.nchains,) if self.batched else ()) + (self.N, self.D))
        _lib.check(_lib.load().kabc_ais_get_ensemble(self._h, x.ctypes.data_as(cd.c_double_p)))
        return x

    def set_timing(self, max_launches, stride=1):
        _lib.check(_lib.load().kabc_ais_set_timing(self._h, int(max_launches)))
        _lib.check(_lib.load().kabc_ais_set_timing_stride(self._h, int(stride)))

    def kernel_ms(self):
        n = C.c_int64()
        ms = _lib.load().kabc_ais_kernel_ms(self._h, C.byref(n))
        return ms, n.value

    def exchange_us(self):
        """kabc_ais_exchange_us: (compute, exchange, exposed) microseconds per half-generation and
        the number of exchange chunks, over the half-generations timed since set_timing (sharded
        handles; zeros otherwise)"""
        out = (C.c_double * 4)()
        _lib.check(_lib.load().kabc_ais_exchange_us(self._h, out))
        return {"compute_us_per_half": out[0], "exchange_us_per_half": out[1],
                "exposed_us_per_half": out[2], "chunks": int(out[3])}

    def set_debug(self, ntransitions):
        _lib.check(_lib.load().kabc_ais_set_debug(self._h, int(ntransitions)))

    def get_debug(self, ntransitions):
        n = self.owned[0] + self.owned[1]
        out = np.empty((n, int(ntransitions), 6), dtype=np.int32)
        _lib.check(_lib.load().kabc_ais_get_debug(
            self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    def close(self):
        if self._h:
            _lib.load().kabc_ais_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chain_seeds(seed, nchains):
    """The per-chain seeds sample(..., MCMCThreads(), Ns, Nc) derives from `seed`
    (AbstractMCMC seeds each chain from the parent rng; here: a golden-ratio stride)."""
    return [(int(seed) + 0x9E3779B97F4A7C15 * (c + 1)) % (1 << 63) for c in range(int(nchains))]


def _bundle(samples, scalar):
    """bundle_samples (src/KissABC.jl:82-94): [Ns][D] -> one Particles per parameter."""
    P = [Particles(samples[:, k]) for k in range(samples.shape[1])]
    return P[0] if (len(P) == 1 or scalar) else P


def _sample_chains(model, N, Ns, seeds, costs, ntransitions, discard_initial, retry_sampling, ctx, ens=None,
                   summary=False, autocorr=None, hist=None, derived=None):
    """len(seeds) independent chains of AIS(N) in ONE batch handle (costs: one DeviceCost per chain, or
    None; ens: that handle where the caller has created it, closed here): the first Ns samples of each,
    [Nc][Ns][D], and the handle's driver; summary: the chains' PosteriorSummary (leading chain axis) in place
    of the samples"""
    Nc, D = len(seeds), len(model)
    if ens is None:
        ens = AisEnsemble(model, N, ctx=ctx, seeds=seeds, costs=costs)
    gk = max(1, -(-Ns // N))
    if summary:
        try:
            return _summarise(ens, gk, N, ntransitions, discard_initial, retry_sampling, autocorr, hist,
                              derived), ens.driver
        finally:
            ens.close()
    big = gk * Nc * N * D * 8 > (1 << 20)   # (a small trace is not worth a helper thread: see sample)
    pool = concurrent.futures.ThreadPoolExecutor(1) if big else None
    buf = pool.submit(_lib.pinned_empty, (gk, Nc, N, D)) if big else None
    try:
        driver = ens.driver
        ens.init(retry_sampling)
        gd = -(-int(discard_initial) // N)
        if gd:
            ens.advance(gd, ntransitions)
        tr = ens.advance(gk, ntransitions,
                         out=buf.result() if big else _lib.pinned_empty((gk, Nc, N, D)))   # [gk][Nc][N][D]
        chains = np.ascontiguousarray(tr.transpose(1, 0, 2, 3)).reshape(Nc, gk * N, D)[:, :Ns]
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
        ens.close()
    return chains, driver


def _summarise(ens, gk, N, ntransitions, discard_initial, retry_sampling, autocorr=None, hist=None, derived=None):
    """sample()'s course on `ens` with the kept generations summarised on the device"""
    ens.init(retry_sampling)
    gd = -(-int(discard_initial) // N)
    if gd:
        ens.advance(gd, ntransitions)
    bkw = {"autocorr": autocorr} if autocorr else {}
    if hist is not None and hist is not False:
        bkw["hist"] = hist
    if derived is not None:
        bkw["derived"] = derived
    ens.summary_begin(**bkw)
    ens.advance(gk, ntransitions, summary=True)
    return ens.summary()


def _chain_kw(kw, c, nchains, D):
    """sample()'s summary keywords for chain c alone: a [chain][D] range of `hist` gives its row c"""
    spec = _hist_spec(kw.get("hist"), "sample")
    if spec is None or spec[1] is None:
        return kw
    row = lambda v: v[c] if v.shape == (nchains, D) else v   # noqa: E731
    return dict(kw, hist=(row(spec[1]), row(spec[2]), spec[0]))


def sample(model, spl, *args, ntransitions=1, discard_initial=0, retry_sampling=100, seed=0,
           progress=False, ctx=None, return_array=False, summary=False, autocorr=None, hist=None, derived=None,
           **kwargs):
    """sample(model, AIS(N), Ns; ...) and sample(model, AIS(N), MCMCThreads(), Ns, Nc; ...).

    The device advances a whole generation (every walker `ntransitions` times) per
    launch pair and a generation yields the N samples the reference's N
    consecutive step() calls would emit (src/KissABC.jl:66-80), so
    ceil(discard_initial/N) generations are discarded and ceil(Ns/N) are kept.

    `summary=True` returns a PosteriorSummary (mean, std, cov, min, max per parameter) accumulated on the
    device in place of the samples: no trace crosses to the host.  It covers the ceil(Ns/N) kept generations
    WHOLE, so its n = ceil(Ns/N) * N, which exceeds Ns where N does not divide it (the samples form keeps the
    first Ns).  With MCMCThreads it returns a ChainSummaries: one PosteriorSummary per chain, `.pooled` and
    `.rhat`.  It excludes return_array.  `autocorr=True` (maxlag = 64) or a maximum lag adds tau, ess and mcse
    per parameter to the summary (per chain with MCMCThreads, whose `.ess` is the chains' sum); it needs
    summary=True.  `hist` (True: 128 bins, an int, (lo, hi) or (lo, hi, nbins): AisEnsemble.summary_begin) adds
    a marginal histogram per parameter and with it quantile(q), median and interval(level); it needs
    summary=True too.  Its automatic range is taken from the walkers after discard_initial -- a convention,
    not a guarantee: `underflow` and `overflow` report what it missed, and a discrete parameter wants an
    explicit integer-aligned range such as (-0.5, K + 0.5, K + 1).  With MCMCThreads every chain has its own
    range, and `.pooled` carries a histogram only for a range the caller gave.  `derived` (a Derived: a C
    snippet mapping a trace row to G quantities) adds `.derived`, a PosteriorSummary of those quantities
    accumulated on the device beside the parameters' (AisEnsemble.summary_begin); it needs summary=True and a
    single-process ensemble.  With MCMCThreads `.derived` is the ChainSummaries of the chains' derived sets and
    `.pooled.derived` its pooled summary.
    """
    if not isinstance(spl, AIS):
        raise TypeError("sampler must be AIS(nparticles)")
    if summary and return_array:
        raise ValueError("sample: summary=True returns moments, not samples; it excludes return_array")
    if _autocorr_maxlag(autocorr, "sample") and not summary:
        raise ValueError("sample: autocorr is part of the device summary; it needs summary=True")
    if _hist_spec(hist, "sample") is not None and not summary:
        raise ValueError("sample: hist is part of the device summary; it needs summary=True")
    akw = {"autocorr": autocorr} if _autocorr_maxlag(autocorr, "sample") else {}
    if _hist_spec(hist, "sample") is not None:
        akw["hist"] = hist
    _derived_check(derived, "sample", summary=summary)
    if derived is not None:
        akw["derived"] = derived
    if args and isinstance(args[0], MCMCThreads):
        # chains are a grid dimension of ONE device handle: every launch advances all Nc
        # ensembles (kabc_ais_create_batch); chain c is bit-identical to a single-chain run
        # with its seed.  A shape the batch handle refuses (KABC_ERR_UNSUPPORTED: beyond KABC_MAX_DIM
        # parameters an ensemble too large for one workgroup's LDS, a user cost) runs the chains one
        # after another with the same seeds: the reference's signature never fails on shape alone.
        # Only the handle's CREATION decides that; an error of init() or advance() is the caller's.
        _, Ns, Nc = args
        Ns, Nc, D = int(Ns), int(Nc), len(model)
        seeds = chain_seeds(seed, Nc)
        try:
            ens = AisEnsemble(model, spl.nparticles, ctx=ctx, seeds=seeds)
        except _lib.KabcError as e:
            if e.status != cd.KABC_ERR_UNSUPPORTED:
                raise
            ens = None
        if summary:
            if ens is not None:
                both, _ = _sample_chains(model, spl.nparticles, Ns, seeds, None, ntransitions,
                                         discard_initial, retry_sampling, ctx, ens=ens, summary=True, **akw)
                return ChainSummaries(both.chain(c) for c in range(Nc))
            return ChainSummaries(sample(model, spl, Ns, ntransitions=ntransitions, discard_initial=discard_initial,
                                         retry_sampling=retry_sampling, seed=sd, ctx=ctx, summary=True,
                                         **_chain_kw(akw, c, Nc, D))
                                  for c, sd in enumerate(seeds))
        if ens is not None:
            chains, _ = _sample_chains(model, spl.nparticles, Ns, seeds, None, ntransitions,
                                       discard_initial, retry_sampling, ctx, ens=ens)
        else:
            chains = np.stack([sample(model, spl, Ns, ntransitions=ntransitions, discard_initial=discard_initial,
                                      retry_sampling=retry_sampling, seed=sd, ctx=ctx, return_array=True)
                               for sd in seeds])
        stacked = chains.reshape(Nc * Ns, D)  # chainsstack, src/KissABC.jl:96-104
        return stacked if return_array else _bundle(stacked, model.scalar)
    (Ns,) = args
    Ns = int(Ns)
    N = spl.nparticles
    ens = AisEnsemble(model, N, seed=seed, ctx=ctx)
    gk = max(1, -(-Ns // N))
    if summary:
        try:
            return _summarise(ens, gk, N, ntransitions, discard_initial, retry_sampling, akw.get("autocorr"),
                              akw.get("hist"), akw.get("derived"))
        finally:
            ens.close()
    shape = (gk, N, len(model))
    # the page-locked trace buffer is allocated on a helper thread (pinning costs
    # ~40 us per MiB) while init and the discarded generations run on the device; a small
    # trace (the reference's own test shapes) is not worth a thread: 0.1-0.2 ms of a 0.5 ms call
    big = gk * N * len(model) * 8 > (1 << 20)
    pool = concurrent.futures.ThreadPoolExecutor(1) if big else None
    buf = pool.submit(_lib.pinned_empty, shape) if big else None
    try:
        ens.init(retry_sampling)
        gd = -(-int(discard_initial) // N)
        if gd:
            ens.advance(gd, ntransitions)
        out = ens.advance(gk, ntransitions, out=buf.result() if big else _lib.pinned_empty(shape))
        out = out.reshape(gk * N, len(model))[:Ns]
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
        ens.close()
    return out if return_array else _bundle(out, model.scalar)


class AisBatchResult(list):
    """sample_batch's result: one entry per run, shaped as sample() returns it, and `.info` about the call."""

    info = None


def _model_difference(m, m0):
    """what sets model m apart from model 0 beyond its cost's params / data, else None"""
    if type(m) is not type(m0):
        return "its class"
    if len(m) != len(m0) or m.scalar != m0.scalar or bytes(m.prior.to_c()) != bytes(m0.prior.to_c()):
        return "its prior"
    if not (m.eps == m0.eps or (math.isnan(m.eps) and math.isnan(m0.eps))):
        return "its eps"
    if m.cost.id != m0.cost.id:
        return "its cost id"
    if m.cost.params.size != m0.cost.params.size or m.cost.data.size != m0.cost.data.size:
        return "its cost's params / data lengths"
    return None


def sample_batch(model, spl, Ns, nruns=None, *, seeds=None, seed=0, ntransitions=1, discard_initial=0,
                 retry_sampling=100, ctx=None, return_array=False, course=None, summary=False, autocorr=None,
                 hist=None, derived=None):
    """One model fitted to many datasets, or one dataset under many seeds, in one call: run r is
    sample(model_r, spl, Ns, seed=seeds[r], <the same keywords>), bit for bit.

    `model` is one model (the runs differ by their seeds only; `nruns` is required) or a sequence of
    models, one per dataset, of one class with the same prior, eps, cost id and cost params / data lengths
    (`nruns` defaults to its length).  `seeds` defaults to chain_seeds(seed, nruns).  With
    length(prior) <= KABC_MAX_DIM the runs are the chains of ONE batch handle (kabc_ais_create_batch_costs:
    info["course"] == "grid", info["driver"] "small" or "halves"); other shapes, and a cost plugin built
    by hipcc whose runs differ in their cost values, run as sample() calls one after another
    ("sequential").  `course` overrides that choice: "grid" asks for the batch handle at any
    length(prior) -- beyond KABC_MAX_DIM it exists for built-in costs and prior families whose ensemble
    fits one workgroup's LDS (csrc/ais_dyn_small_kernel.hpp) -- and raises KabcError where the shape is
    refused; "sequential" forces the loop of sample() calls.  Same bits on either course.  Returns a list with one entry per run; its `.info` holds the course, the driver,
    nruns and the wall time.  `summary=True` gives one PosteriorSummary per run in place of its samples, on
    either course (sample's own summary=True: n = ceil(Ns/N) * N per run; `autocorr`, `hist` and `derived` as in sample, a [run][D] range of `hist` giving run r its row).  A failed initial draw raises KabcError("run r: <the reference's message>");
    Context.cancel() / Ctrl-C behave as they do for sample()."""
    if not isinstance(spl, AIS):
        raise TypeError("sampler must be AIS(nparticles)")
    if course not in (None, "grid", "sequential"):
        raise ValueError(f'sample_batch: course must be None, "grid" or "sequential", not {course!r}')
    if summary and return_array:
        raise ValueError("sample_batch: summary=True returns moments, not samples; it excludes return_array")
    if _autocorr_maxlag(autocorr, "sample_batch") and not summary:
        raise ValueError("sample_batch: autocorr is part of the device summary; it needs summary=True")
    if _hist_spec(hist, "sample_batch") is not None and not summary:
        raise ValueError("sample_batch: hist is part of the device summary; it needs summary=True")
    _derived_check(derived, "sample_batch", summary=summary)
    if isinstance(model, _ApproxModel):
        if nruns is None:
            raise ValueError("sample_batch: nruns is required with a single model")
        nruns = int(nruns)
        models = [model] * max(nruns, 0)
    else:
        models = list(model)
        if not all(isinstance(m, _ApproxModel) for m in models):
            raise TypeError("sample_batch: `model` must be a model or a sequence of models")
        nruns = len(models) if nruns is None else int(nruns)
        if len(models) != nruns:
            raise ValueError(f"sample_batch: {len(models)} models for nruns = {nruns}")
    if nruns < 1:
        raise ValueError("sample_batch: nruns must be >= 1")
    m0 = models[0]
    for r, m in enumerate(models):
        if m is not m0:
            what = _model_difference(m, m0)
            if what:
                raise ValueError(f"sample_batch: model {r} differs from model 0 in {what}")
    seeds = chain_seeds(seed, nruns) if seeds is None else [int(x) for x in seeds]
    if len(seeds) != nruns:
        raise ValueError(f"sample_batch: len(seeds) = {len(seeds)} != nruns = {nruns}")
    Ns, N, D = int(Ns), spl.nparticles, len(m0)
    kw = dict(ntransitions=ntransitions, discard_initial=discard_initial, retry_sampling=retry_sampling)
    skw = {"summary": True} if summary else {}
    if summary and _autocorr_maxlag(autocorr, "sample_batch"):
        skw["autocorr"] = autocorr
    if summary and _hist_spec(hist, "sample_batch") is not None:
        skw["hist"] = hist
    if derived is not None:
        skw["derived"] = derived
    t0 = time.perf_counter()
    chains, driver = None, None
    if course == "grid" or (course is None and D <= cd.KABC_MAX_DIM):
        try:
            chains, driver = _sample_chains(m0, N, Ns, seeds, [m.cost for m in models], ctx=ctx, **kw, **skw)
        except _lib.Cancelled:
            raise
        except _lib.KabcError as e:
            msg = str(e)
            if msg.startswith("chain "):   # (a failed initial draw: "chain r: ...")
                raise _lib.KabcError(e.status, "run " + msg[len("chain "):]) from None
            if e.status != cd.KABC_ERR_UNSUPPORTED or course == "grid":
                raise
            # (a shape the batch handle refuses: the runs one after another, each with sample()'s own checks)
    if chains is not None and summary:
        out = AisBatchResult(chains.chain(r) for r in range(nruns))
        course = "grid"
    elif chains is not None:
        out = AisBatchResult(c if return_array else _bundle(c, m0.scalar) for c in chains)
        course = "grid"
    else:
        out = AisBatchResult()
        for r, m in enumerate(models):
            try:
                out.append(sample(m, spl, Ns, seed=seeds[r], ctx=ctx, return_array=return_array, **kw,
                                  **_chain_kw(skw, r, nruns, D)))
            except _lib.Cancelled:
                raise
            except _lib.KabcError as e:
                raise _lib.KabcError(e.status, f"run {r}: {e}") from None
        course, driver = "sequential", "halves"   # (each run on the driver its own handle picks)
    out.info = {"course": course, "driver": driver, "nruns": nruns,
                "wall_ms": (time.perf_counter() - t0) * 1e3}
    return out


class SmcResult(collections.namedtuple("SmcResult", ["P", "C", "eps", "info"])):
    """(P, C, ϵ) of src/smc.jl:205 (+ info); `.ϵ`/`.ε` alias `.eps`."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ("\u03b5", "\u03f5"):
            return self.eps
        raise AttributeError(name)


_SMC_LOG_KEYS = ("eps", "ess", "accepted", "resampled", "flag", "passes")


class SmcState:
    """What an smc run holds at an iteration boundary (kabc_smc_state_t, include/kabc.h): enough to go on
    from there with `smc(prior, cost, resume=state, ...)`, bit for bit as if the run had never stopped --
    given the same prior, cost, seed and options.  `theta` [N][D] holds the walkers as the loop holds them,
    NOT push_p'ed (a discrete prior's walkers sit between integers); `cost`, `logprior` [N] and `alive`
    [N] belong to them.  `iteration` counts the completed iterations, `pass_count` the propose / accept
    passes (the transition counter of the random streams), `log` holds the records of those iterations.
    `save(path)` / `load(path)`: one .npz of arrays and scalars, no pickle."""

    _INTS = ("seed", "iteration", "pass_count", "accepted", "cost_evals", "proposals", "n_alive")
    _UNSIGNED = ("seed", "pass_count", "accepted", "cost_evals", "proposals")

    def __init__(self, theta, cost, logprior, alive, *, seed, iteration, pass_count, eps, eps_prev,
                 accepted, cost_evals, proposals, n_alive, log=()):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64)
        if self.theta.ndim != 2:
            raise ValueError("SmcState: theta must be [nparticles][D]")
        n = self.theta.shape[0]
        self.cost = np.ascontiguousarray(cost, dtype=np.float64).reshape(-1)
        self.logprior = np.ascontiguousarray(logprior, dtype=np.float64).reshape(-1)
        self.alive = np.ascontiguousarray(alive, dtype=np.uint8).reshape(-1)
        for name in ("cost", "logprior", "alive"):
            if getattr(self, name).shape[0] != n:
                raise ValueError(f"SmcState: {name} has {getattr(self, name).shape[0]} entries for {n} particles")
        for name in self._INTS:
            setattr(self, name, int(locals()[name]))
        self.eps, self.eps_prev = float(eps), float(eps_prev)
        self.log = [dict(rec) for rec in log]

    nparticles = property(lambda self: self.theta.shape[0])
    D = property(lambda self: self.theta.shape[1])

    def save(self, path):
        """Write the state to `path` as one .npz (the name is used as given)."""
        arrays = {"theta": self.theta, "cost": self.cost, "logprior": self.logprior, "alive": self.alive,
                  "eps": np.float64(self.eps), "eps_prev": np.float64(self.eps_prev)}
        for name in self._INTS:
            arrays[name] = (np.uint64 if name in self._UNSIGNED else np.int64)(getattr(self, name))
        for key in _SMC_LOG_KEYS:
            arrays["log_" + key] = np.array([rec[key] for rec in self.log],
                                            dtype=np.float64 if key == "eps" else np.int64)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cols = {key: z["log_" + key] for key in _SMC_LOG_KEYS}
            log = [{key: (float(cols[key][i]) if key == "eps" else int(cols[key][i])) for key in _SMC_LOG_KEYS}
                   for i in range(len(cols["eps"]))]
            return cls(z["theta"], z["cost"], z["logprior"], z["alive"], eps=float(z["eps"]),
                       eps_prev=float(z["eps_prev"]), log=log, **{name: int(z[name]) for name in cls._INTS})

    def _to_c(self):
        st = cd.SmcState()
        st.nparticles, st.D, st.seed = self.nparticles, self.D, self.seed
        st.iteration, st.pass_, st.eps, st.eps_prev = self.iteration, self.pass_count, self.eps, self.eps_prev
        st.accepted, st.cost_evals, st.proposals, st.n_alive = self.accepted, self.cost_evals, self.proposals, self.n_alive
        st.theta = self.theta.ctypes.data_as(cd.c_double_p)
        st.cost = self.cost.ctypes.data_as(cd.c_double_p)
        st.logprior = self.logprior.ctypes.data_as(cd.c_double_p)
        st.alive = self.alive.ctypes.data_as(C.POINTER(C.c_uint8))
        return st


def smc(prior, cost, *, nparticles=None, alpha=0.95, mcmc_retrys=0, mcmc_tol=0.015, epstol=0.0,
        r_epstol=None, min_r_ess=None, max_stretch=2.0, verbose=False, parallel=False, seed=None,
        ctx=None, return_array=False, comm=None, shard=None, max_iterations=None, return_state=False,
        resume=None):
    """smc(prior, cost; ...) -- src/smc.jl:92-206, same keywords and defaults (nparticles = 100, seed = 0).
    `parallel` is accepted and ignored (every particle is a GPU lane).
    `comm` (a comm.Comm): the cost loop is sharded over the communicator's ranks
    (kabc_smc_run_dist -- the reference's `parallel = true` leg across GPUs, for expensive
    simulators); collective, every rank gets the same result, equal to the single-GPU one.
    `shard` = "particles": the ranks own their particles and the epsilon-selection is sharded too
    (kabc_smc_run_dist_mode, KABC_SMC_DIST_PARTICLES); "cost_loop": the pass only; None:
    kabc_smc_run_dist's default (KABC_SMC_DIST).
    `max_iterations` bounds the outer loop (default 100 000).  Context.cancel() or Ctrl-C stops a
    single-GPU run at an iteration boundary: Cancelled (its `.result` holds the population after the
    iterations that completed) or KeyboardInterrupt.
    `return_state=True` (kabc_smc_run_from): info["state"] is the SmcState the run ended in -- also on
    Cancelled.result.  `resume=state` continues from it instead of drawing from the prior: `nparticles`
    and `seed` default to the state's; iterations, cost_evals, proposals and `max_iterations` count from
    the start of the run; info["log"] is the state's log followed by this call's records, and
    info["first_iteration"] tells where this call began (with a state in or out the log holds every
    iteration; a plain call keeps its first 4096 records).  With the same prior, cost, seed and options
    the continued run is the uninterrupted one, bit for bit.  The stop tests are applied to the state
    first: a run that ended by rule stays as it is under the same options and goes on under a smaller
    `epstol`; one stopped by `max_iterations` or a cancel goes on.  Single GPU only (no `comm`).
    Returns (P, C, ϵ) as the reference does (+ an `info` dict)."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if comm is not None and (resume is not None or return_state):
        raise ValueError("smc: resume= and return_state= are single-GPU only (no comm=)")
    if resume is not None:
        if not isinstance(resume, SmcState):
            raise TypeError("smc: resume must be an SmcState")
        if nparticles is not None and int(nparticles) != resume.nparticles:
            raise ValueError(f"smc: nparticles = {int(nparticles)}, the state holds {resume.nparticles} particles")
        if len(fac) != resume.D:
            raise ValueError(f"smc: length(prior) = {len(fac)}, the state's walkers have {resume.D} parameters")
        nparticles = resume.nparticles
        seed = resume.seed if seed is None else seed
    nparticles = 100 if nparticles is None else nparticles
    seed = 0 if seed is None else seed
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.SmcOpts()
    lib.kabc_smc_default_opts(C.byref(o))
    o.nparticles = int(nparticles)
    o.alpha = float(alpha)
    o.mcmc_retrys = int(mcmc_retrys)
    o.verbose = int(bool(verbose))
    o.mcmc_tol = float(mcmc_tol)
    o.epstol = float(epstol)
    o.r_epstol = math.nan if r_epstol is None else float(r_epstol)
    o.min_r_ess = math.nan if min_r_ess is None else float(min_r_ess)
    o.max_stretch = float(max_stretch)
    o.seed = int(seed)
    if max_iterations is not None:   # (kabc_smc_opts_t.max_iterations: the loop's safety bound, 100 000)
        o.max_iterations = int(max_iterations)
    N, D = int(nparticles), len(fac)
    n_alloc = max(N, 1)
    t_host0 = time.perf_counter()
    theta = _lib.result_empty((n_alloc, D))
    Cst = _lib.result_empty(n_alloc)
    alive = np.zeros(n_alloc, dtype=np.uint8)
    # the log: 4096 records; with a state in or out, every iteration this call can run -- a state's log has
    # no gaps, its record i is iteration i + 1
    log_cap = 4096
    if return_state or resume is not None:
        first = resume.iteration if resume is not None else 0
        log_cap = max((o.max_iterations if o.max_iterations > 0 else 100000) - first, 1)
    log = (cd.SmcIter * log_cap)()
    r = cd.SmcResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    r.alive = alive.ctypes.data_as(C.POINTER(C.c_uint8))
    r.iter_log = log
    r.iter_log_cap = log_cap
    cc = cost.to_c()
    if shard not in (None, "cost_loop", "particles"):
        raise ValueError('shard is None, "cost_loop" or "particles"')
    if comm is not None and shard is not None:
        _lib.check(lib.kabc_smc_run_dist_mode(comm.handle, fac.to_c(), D, C.byref(cc), C.byref(o),
                                              1 if shard == "particles" else 0, C.byref(r)))
    elif comm is not None:
        _lib.check(lib.kabc_smc_run_dist(comm.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r)))
    else:
        # (a state in or out: kabc_smc_run_from; else kabc_smc_run, which copies nothing more)
        to = st_from = st_to = None
        if return_state:
            to = SmcState(np.empty((n_alloc, D)), np.empty(n_alloc), np.empty(n_alloc), np.zeros(n_alloc, np.uint8),
                          seed=0, iteration=-1, pass_count=0, eps=math.inf, eps_prev=math.inf, accepted=0,
                          cost_evals=0, proposals=0, n_alive=0)
            st_to = to._to_c()
        if resume is not None:
            st_from = resume._to_c()
        with ctx.interruptible():
            if to is None and resume is None:
                status = lib.kabc_smc_run(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r))
            else:
                status = lib.kabc_smc_run_from(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o),
                                               C.byref(st_from) if st_from is not None else None,
                                               C.byref(st_to) if st_to is not None else None, C.byref(r))
            if status == cd.KABC_ERR_CANCELLED:
                # the population after the iterations that completed travels with the exception
                try:
                    _lib.check(status)
                except _lib.Cancelled as e:
                    e.result = _smc_result(lib, r, theta, Cst, alive, log, n_alloc, N, return_array,
                                           scalar, t_host0, time.perf_counter(), resume, to, st_to)
                    raise
            _lib.check(status)
        return _smc_result(lib, r, theta, Cst, alive, log, n_alloc, N, return_array, scalar, t_host0,
                           time.perf_counter(), resume, to, st_to)
    return _smc_result(lib, r, theta, Cst, alive, log, n_alloc, N, return_array, scalar, t_host0,
                       time.perf_counter())


def _smc_result(lib, r, theta, Cst, alive, log, n_alloc, N, return_array, scalar, t_host0, t_host1,
                resume=None, to=None, st_to=None):
    mask = alive.view(np.bool_)          # (the library writes 0 / 1)
    # every particle alive (the usual end of a run): the result IS the array, not a gathered copy
    kept = theta if (r.n_alive == n_alloc and N > 0) else theta[mask]
    first = resume.iteration if resume is not None else 0   # (the library's log holds this call's iterations)
    nit = min(r.iterations - first, len(log))
    info = {
        "iterations": r.iterations, "n_alive": r.n_alive, "cost_evals": r.cost_evals,
        "proposals": r.proposals, "alive": mask, "theta_all": theta,
        "kernel_ms_mcmc": r.kernel_ms_mcmc, "mcmc_launches": r.mcmc_launches,
        "log": [dict(eps=log[i].eps, ess=log[i].ess, accepted=log[i].accepted,
                     resampled=log[i].resampled, flag=log[i].flag, passes=log[i].mcmc_passes)
                for i in range(nit)],
    }
    if resume is not None:
        info["log"] = [dict(rec) for rec in resume.log] + info["log"]
        info["first_iteration"] = first
    if to is not None:   # the scalars the library wrote into the struct; the arrays it filled in place
        for name in SmcState._INTS:
            setattr(to, name, int(getattr(st_to, "pass_" if name == "pass_count" else name)))
        to.eps, to.eps_prev = st_to.eps, st_to.eps_prev
        to.log = [dict(rec) for rec in info["log"]]
        info["state"] = to
    if True:   # how the run was driven (kabc_smc_dist_stats)
        ds = (C.c_int64 * 8)()
        lib.kabc_smc_dist_stats(ds)
        info["dist"] = {"iterations": ds[0], "collectives": ds[1], "host_looks": ds[2],
                        "one_exchange_selections": ds[3], "phase_by_phase_selections": ds[4],
                        "passes": ds[5], "batched": bool(ds[6]), "collectives_per_usual_iteration": ds[7],
                        "collectives_per_iteration": round(ds[1] / max(ds[0], 1), 3)}
    P = kept if return_array else _bundle(kept, scalar)
    # where the wall time of this call went: kabc_smc_run (with its result copy) / this wrapper
    info["host_ms"] = {"kabc_smc_run": (t_host1 - t_host0) * 1e3,
                       "python_after": (time.perf_counter() - t_host1) * 1e3}
    return SmcResult(P, Cst, r.eps, info)


PriorPredictiveResult = collections.namedtuple("PriorPredictiveResult", ["P", "C", "logprior", "info"])


def prior_predictive(prior, cost, n, nrep=None, seed=0, first_row=0, ctx=None, return_array=False):
    """The pilot simulation `cost.(rand(prior) for _ in 1:n)` in one call (kabc_prior_predictive,
    include/kabc.h): n draws push_p(prior, rand(prior)), their log-prior and their costs, nrep
    replicates each, without θ visiting the host in between -- where the reference picks the ϵ its
    samplers ask for: `np.quantile(prior_predictive(prior, cost, 10_000).C, 0.01)`.

    Returns (P, C, logprior, info): `P` bundled like smc's (one Particles per parameter, or the [n][D]
    array with `return_array`), `C` [n] (`nrep=None`) or [n][nrep], `logprior` [n].  Row i is the draw
    `kabc_factored_rand(seed, DOM_EVAL_DRAW, first_walker = first_row + i)`, and
    `C == cost.evaluate(P, nrep, seed, first_row)` bit for bit."""
    from .costs import check_eval_args
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    n, D = int(n), len(fac)
    check_eval_args(cost, D, nrep, first_row, n)
    R = 1 if nrep is None else int(nrep)
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    t0 = time.perf_counter()
    theta = _lib.result_empty((n, D))
    lp = _lib.result_empty(n)
    Cst = _lib.result_empty((n, R))
    cc = cost.to_c()
    with ctx.interruptible():
        _lib.check(lib.kabc_prior_predictive(ctx.handle, fac.to_c(), D, C.byref(cc), n, R, int(seed), int(first_row),
                                             theta.ctypes.data_as(cd.c_double_p), lp.ctypes.data_as(cd.c_double_p),
                                             Cst.ctypes.data_as(cd.c_double_p)))
    st = (C.c_double * 4)()
    lib.kabc_eval_stats(st)
    info = {"launches": int(st[1]), "rows_per_launch": int(st[3]), "kernel_ms": st[0], "prior_kernel_ms": st[2],
            "wall_ms": (time.perf_counter() - t0) * 1e3}
    if nrep is None:
        Cst = Cst[:, 0]
    return PriorPredictiveResult(theta if return_array else _bundle(theta, scalar), Cst, lp, info)


class RejectResult(collections.namedtuple("RejectResult", ["P", "C", "logprior", "eps", "info"])):
    """abc_reject's result; `.ϵ`/`.ε` alias `.eps`."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ("\u03b5", "\u03f5"):
            return self.eps
        raise AttributeError(name)


def abc_reject(prior, cost, eps=None, n=None, *, draws=None, keep=None, seed=0, first_row=0, ctx=None,
               return_array=False):
    """Rejection ABC on the GPU (kabc_abc_reject, include/kabc.h): draw from the prior, simulate, keep the
    draw if `cost <= eps` -- the accepted draws are independent draws from prior x 1[cost <= eps].

    `abc_reject(prior, cost, eps, n)`: the first `n` accepted rows in index order; `draws=` bounds the rows
    drawn (default: the whole stream, 2^32 - first_row).  Fewer than n acceptances within the budget is no
    error: `info["exhausted"]`.  `abc_reject(prior, cost, draws=N, keep=k)`: the k rows with the smallest
    (cost, index) of N draws (NaN costs excluded), in index order; `eps` of the result is the largest kept
    cost -- the reference's `quantile` then `Xs .<= ϵ` (src/smc.jl:134-139) on a pilot run.

    Row i is row i of `prior_predictive(prior, cost, draws, seed=seed, first_row=first_row)`, bit for bit;
    `info["index"]` holds the i of every returned row.  Rows are drawn, simulated, tested and compacted on
    the device: only accepted rows cross PCIe.  Returns (P, C, logprior, eps, info): `P` bundled like
    smc's (or the [n_out][D] array with `return_array`); info: index, draws, accepted_seen, exhausted,
    course ("fused" / "phases"), launches, kernel_ms (KABC_EVAL_TIMING=1), wall_ms, acceptance = n_out / draws.
    Context.cancel() / Ctrl-C: Cancelled (its `.result` holds what the completed rows gave) /
    KeyboardInterrupt."""
    from .costs import check_reject_args
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    D = len(fac)
    n_accept, max_draws, k = check_reject_args(cost, D, eps, n, draws, keep, first_row)
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    t0 = time.perf_counter()
    o = cd.RejectOpts()
    lib.kabc_reject_default_opts(C.byref(o))
    if not k:
        o.eps = float(eps)
    o.n_accept, o.max_draws, o.keep, o.seed, o.first_row = n_accept, max_draws, k, int(seed), int(first_row)
    cap = max(n_accept, k)
    theta = _lib.result_empty((cap, D))
    Cst, lp = _lib.result_empty(cap), _lib.result_empty(cap)
    index = np.empty(cap, dtype=np.int64)
    r = cd.RejectResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    r.logprior = lp.ctypes.data_as(cd.c_double_p)
    r.index = index.ctypes.data_as(C.POINTER(C.c_int64))
    r.capacity = cap
    cc = cost.to_c()

    def result():
        m = int(r.n_out)
        info = {"index": index[:m], "draws": int(r.draws), "accepted_seen": int(r.accepted_seen),
                "exhausted": bool(r.exhausted), "course": "phases" if r.course else "fused",
                "launches": int(r.launches), "kernel_ms": r.kernel_ms, "wall_ms": (time.perf_counter() - t0) * 1e3,
                "acceptance": m / r.draws if r.draws else math.nan}
        P = theta[:m]
        return RejectResult(P if return_array else _bundle(P, scalar), Cst[:m], lp[:m], r.eps, info)

    with ctx.interruptible():
        status = lib.kabc_abc_reject(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r))
        if status == cd.KABC_ERR_CANCELLED:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = result()
                raise
        _lib.check(status)
    return result()


class PmcResult(collections.namedtuple("PmcResult", ["theta", "w", "C", "logprior", "eps", "info"])):
    """abc_pmc's result: the last complete generation as a weighted sample -- `theta` [N][D], normalised weights
    `w`, costs `C`, `logprior`, its `eps`; `.mean` / `.cov` are its weighted moments, `.ess` = 1 / sum w^2;
    `.ϵ`/`.ε` alias `.eps`."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ("\u03b5", "\u03f5"):
            return self.eps
        if name in ("mean", "cov"):
            return self.info[name]
        if name == "ess":
            return float(1.0 / np.sum(self.w * self.w)) if self.w.size else math.nan
        raise AttributeError(name)

    def resample(self, n=None, seed=0):
        """`n` (default N) equally weighted draws from the weighted sample, bundled like smc's `P` (one
        Particles per parameter).  A host resample with numpy's generator: a convenience, not part of the
        bit contract."""
        n = len(self.w) if n is None else int(n)
        pick = np.random.default_rng(seed).choice(len(self.w), size=n, p=self.w / self.w.sum())
        return _bundle(self.theta[pick], self.info["scalar"])


def abc_pmc(prior, cost, nparticles, *, eps=None, q=None, eps0=math.inf, eps_target=-math.inf, generations=None,
            kernel="full", scale=2.0, max_draws=None, min_rate=0.0, seed=0, ctx=None):
    """ABC population Monte Carlo on the GPU (Beaumont, Cornuet, Marin, Robert 2009; kabc_abc_pmc,
    include/kabc.h): a sequence of rejection samplers, each proposing from a Gaussian mixture around the
    previous population, with importance weights -- every generation is a weighted sample of
    prior x 1[cost <= eps_g].  Generation 0 is `abc_reject(prior, cost, eps_0, nparticles, seed=seed)`.

    Schedule: `eps=[...]` runs one generation per entry; without it the schedule is adaptive --
    eps_0 = `eps0`, eps_g = max(eps_target, quantile(C_{g-1}, q)) (q = 0.5), at most `generations` (20)
    generations, stopping at `eps_target` or when the quantile no longer falls.  `kernel`: "full" (scale x
    the weighted covariance) or "diag".  `max_draws` bounds the proposals of ONE generation
    (min(2^32, 10 000 N)); a generation that cannot be filled ends the run with the one before
    (`info["stop"] == "exhausted"`), as does a singular covariance ("degenerate").  `min_rate`: stop after a
    generation that accepted fewer than this share of its proposals.

    Returns PmcResult(theta, w, C, logprior, eps, info); info: log (eps, draws, ess, launches per generation),
    stop, generations_run, index (each particle's row in its generation's proposal stream:
    `cost.evaluate(theta[i], nrep=g + 1, seed=seed, first_row=index[i])[g]` is C[i]), course, mean, cov, kernel_ms
    and its parts proposal_kernel_ms / weight_kernel_ms (KABC_EVAL_TIMING=1), host_rules_ms, wall_ms.  Context.cancel() / Ctrl-C: Cancelled (its `.result` is the last complete generation) /
    KeyboardInterrupt."""
    from .costs import check_pmc_args
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    D = len(fac)
    N, eps_a, qv, G, kid, M = check_pmc_args(cost, fac, nparticles, eps, q, eps0, eps_target, generations, kernel,
                                             scale, max_draws, min_rate)
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    t0 = time.perf_counter()
    o = cd.PmcOpts()
    lib.kabc_pmc_default_opts(C.byref(o))
    o.nparticles, o.generations, o.scale, o.min_rate, o.max_draws = N, G, float(scale), float(min_rate), M
    o.kernel, o.seed = kid, int(seed)
    if eps_a is not None:
        o.eps = eps_a.ctypes.data_as(cd.c_double_p)
    else:
        o.eps0, o.eps_target, o.q = float(eps0), float(eps_target), qv
    theta = _lib.result_empty((N, D))
    w, Cst, lp = _lib.result_empty(N), _lib.result_empty(N), _lib.result_empty(N)
    index = np.empty(N, dtype=np.int64)
    mean, cov = np.full(D, math.nan), np.full((D, D), math.nan)
    log = (cd.PmcGen * G)()
    r = cd.PmcResult()
    r.theta, r.w = theta.ctypes.data_as(cd.c_double_p), w.ctypes.data_as(cd.c_double_p)
    r.cost, r.logprior = Cst.ctypes.data_as(cd.c_double_p), lp.ctypes.data_as(cd.c_double_p)
    r.index = index.ctypes.data_as(C.POINTER(C.c_int64))
    r.log = log
    r.mean, r.cov = mean.ctypes.data_as(cd.c_double_p), cov.ctypes.data_as(cd.c_double_p)
    cc = cost.to_c()

    def result():
        g = int(r.generations_run)
        m = N if g else 0
        st = (C.c_double * 4)()
        lib.kabc_pmc_stats(st)
        info = {"log": [dict(eps=log[i].eps, draws=int(log[i].draws), ess=log[i].ess, launches=int(log[i].launches))
                        for i in range(g)],
                "stop": cd.PMC_STOP_NAMES[r.stop], "generations_run": g, "index": index[:m],
                "course": "phases" if r.course else "fused", "mean": mean, "cov": cov, "kernel_ms": r.kernel_ms,
                "proposal_kernel_ms": st[0], "weight_kernel_ms": st[1], "host_rules_ms": st[2],
                "weight_launches": int(st[3]), "wall_ms": (time.perf_counter() - t0) * 1e3, "scalar": scalar}
        return PmcResult(theta[:m], w[:m], Cst[:m], lp[:m], r.eps, info)

    with ctx.interruptible():
        status = lib.kabc_abc_pmc(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r))
        if status == cd.KABC_ERR_CANCELLED:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = result()
                raise
        _lib.check(status)
    return result()


class RejectBatchResult(list):
    """abc_reject_batch's result: one RejectResult per run (a list), and `.info` about the whole call."""

    info = None


_REJECT_BATCH_COURSES = {0: "table", 1: "grid", 2: "sequential"}


def abc_reject_batch(prior, costs, eps=None, n=None, nruns=None, *, seeds=None, seed=0, draws=None, keep=None,
                     first_row=0, ctx=None, return_array=False):
    """Rejection ABC for many datasets in one call (kabc_abc_reject_batch, include/kabc.h): run r is
    `abc_reject(prior, costs[r], eps[r], n, draws=draws, keep=keep, seed=seeds[r], first_row=first_row)`,
    bit for bit -- P, C, logprior, eps and info's index / draws / exhausted.

    `costs` is a sequence of DeviceCosts, one per dataset, with the same cost id and the same params / data
    lengths, or one DeviceCost with `nruns` (or `seeds`): the runs then differ by seed or eps only.  `eps` is a
    number or one per run.  `seeds=None`: every run uses `seed`.

    Runs that share a seed share their θ draws AND the simulator's noise: row i of every such run is the
    same draw of the prior, evaluated against each dataset -- the reference table of rejection ABC, drawn and
    scored once (info["course"] == "table").  These are common random numbers: each run is a valid rejection
    sample for its dataset, but the runs are NOT independent of each other.  `seeds=chain_seeds(seed, nruns)`
    gives independent runs (info["course"] == "grid": one launch grid, nothing else shared).  Shapes the
    batch kernel does not take -- user prior families, MvNormal, very long rows, user costs -- and
    KABC_REJECT_BATCH=0 run one after another ("sequential").  Same bits on every course.

    Returns a RejectBatchResult: a list of RejectResult, entry r as abc_reject returns it (launches and
    kernel_ms of an entry are the whole batch's on the table and grid courses); `.info` holds course, launches,
    runs_per_launch, rows_drawn (θ rows drawn over all launches), nruns, status, wall_ms, kernel_ms
    (KABC_EVAL_TIMING=1).  Context.cancel() / Ctrl-C: Cancelled (its `.result` is the list, every run holding
    what its completed rows gave) / KeyboardInterrupt; any other failure: KabcError("run r: ...")."""
    from .costs import check_reject_batch_args
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    D = len(fac)
    cost_list, seeds, eps_list, n_accept, max_draws, k = check_reject_batch_args(
        costs, D, eps, n, nruns, seeds, draws, keep, first_row)
    R = len(cost_list)
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    t0 = time.perf_counter()
    o = cd.RejectOpts()
    lib.kabc_reject_default_opts(C.byref(o))
    if eps_list:
        o.eps = eps_list[0]
    o.n_accept, o.max_draws, o.keep, o.seed, o.first_row = n_accept, max_draws, k, int(seed), int(first_row)
    cap = max(n_accept, k)
    theta = _lib.result_empty((R, cap, D))
    Cst, lp = _lib.result_empty((R, cap)), _lib.result_empty((R, cap))
    index = np.empty((R, cap), dtype=np.int64)
    # the R result records, written through a uint64 view (the fields set here are 8 bytes wide)
    res = (cd.RejectResult * R)()
    w = np.frombuffer(res, dtype=np.uint64).reshape(R, C.sizeof(cd.RejectResult) // 8)
    rr = np.arange(R, dtype=np.uint64)
    col = lambda f: getattr(cd.RejectResult, f).offset // 8   # noqa: E731
    w[:, col("theta")] = np.uint64(theta.ctypes.data) + rr * np.uint64(cap * D * 8)
    w[:, col("cost")] = np.uint64(Cst.ctypes.data) + rr * np.uint64(cap * 8)
    w[:, col("logprior")] = np.uint64(lp.ctypes.data) + rr * np.uint64(cap * 8)
    w[:, col("index")] = np.uint64(index.ctypes.data) + rr * np.uint64(cap * 8)
    w[:, col("capacity")] = np.uint64(cap)
    cc_of = {}   # (one record per distinct DeviceCost: a repeated one points at the same params)
    for c in cost_list:
        if id(c) not in cc_of:
            cc_of[id(c)] = c.to_c()
    ccs = (cd.Cost * R)(*[cc_of[id(c)] for c in cost_list])
    sd = (C.c_uint64 * R)(*seeds) if seeds is not None else None
    ev = (C.c_double * R)(*eps_list) if eps_list else None
    st = (C.c_int * R)()
    with ctx.interruptible():
        status = lib.kabc_abc_reject_batch(ctx.handle, fac.to_c(), D, ccs, R, sd, ev, C.byref(o), res, st)
        t1 = time.perf_counter()
        bs = (C.c_int64 * 4)()
        lib.kabc_reject_batch_stats(bs)

        def entry(r):
            x = res[r]
            m = int(x.n_out)
            info = {"index": index[r, :m], "draws": int(x.draws), "accepted_seen": int(x.accepted_seen),
                    "exhausted": bool(x.exhausted), "course": "phases" if x.course else "fused",
                    "launches": int(x.launches), "kernel_ms": x.kernel_ms,
                    "acceptance": m / x.draws if x.draws else math.nan}
            P = theta[r, :m]
            return RejectResult(P if return_array else _bundle(P, scalar), Cst[r, :m], lp[r, :m], x.eps, info)

        out = RejectBatchResult(entry(r) for r in range(R))
        kms = [res[r].kernel_ms for r in range(R)]
        out.info = {"course": _REJECT_BATCH_COURSES.get(int(bs[0]), int(bs[0])), "launches": int(bs[1]),
                    "runs_per_launch": int(bs[2]), "rows_drawn": int(bs[3]), "nruns": R,
                    "status": [int(x) for x in st], "wall_ms": (t1 - t0) * 1e3,
                    "kernel_ms": (sum(kms) if bs[0] == 2 else kms[0]) if kms[0] >= 0 else -1.0}
        if status != 0:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = out
                raise
            except _lib.KabcError as e:
                e.results = out
                raise
        return out


class SmcBatchResult(list):
    """smc_batch's result: one SmcResult per run (a list), and `.info` about the whole call."""

    info = None


class _RunInfo(dict):
    """info of one smc_batch run: "log" is built from the batch's iteration-log block on first access"""

    def __missing__(self, key):
        if key != "log":
            raise KeyError(key)
        rows = self._log_rows
        v = self["log"] = [dict(eps=float(e["eps"]), ess=int(e["ess"]), accepted=int(e["accepted"]),
                                resampled=int(e["resampled"]), flag=int(e["flag"]), passes=int(e["mcmc_passes"]))
                           for e in rows]
        return v


_SMC_BATCH_LOG_BYTES = 64 << 20   # the default log cap keeps nruns x log_cap x 40 B within this


def smc_batch(prior, cost, nruns=None, *, seeds=None, seed=0, nparticles=100, alpha=0.95, mcmc_retrys=0,
              mcmc_tol=0.015, epstol=0.0, r_epstol=None, min_r_ess=None, max_stretch=2.0, verbose=False,
              parallel=False, max_iterations=None, log_cap=None, ctx=None, return_array=False, comm=None,
              shard=None):
    """Many independent smc runs in one call (kabc_smc_run_batch): run r is
    smc(prior, cost_r, seed=seeds[r], <the same keywords>), bit for bit.

    `cost` is one DeviceCost (the runs differ by their seeds only; `nruns` is required) or a sequence
    of DeviceCosts, one per dataset, with the same cost id and the same params and data lengths
    (`nruns` defaults to its length).  `seeds` defaults to chain_seeds(seed, nruns).  With
    nparticles <= 256 and length(prior) <= KABC_MAX_DIM the runs are the workgroups of ONE launch grid
    (info["course"] == "grid"); other shapes run one after another ("sequential").  `verbose`, `comm`
    and `shard` are refused.  `log_cap` bounds each run's iteration log; the default is
    min(4096, 64 MiB / (40 B x nruns)) entries, so that the logs of a batch stay within 64 MiB.

    Returns a list of SmcResult, entry r as smc returns it (its P / theta_all / C / alive are views
    into one [nruns][N][D] / [nruns][N] block; info["kernel_ms_mcmc"] is the batch's); the list's
    `.info` holds the course, the kernel launches, the runs per launch and the wall time.  A failed
    run raises KabcError("run r: <the reference's message>") whose `.results` is the list with None at
    the failed runs; Context.cancel() / Ctrl-C raise Cancelled whose `.result` is the list of the runs'
    populations after the iterations they completed (None for runs never started)."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if isinstance(cost, DeviceCost):
        if nruns is None:
            raise ValueError("smc_batch: nruns is required with a single DeviceCost")
        nruns = int(nruns)
        cost_list = [cost] * max(nruns, 0)
    else:
        cost_list = list(cost)
        if not all(isinstance(c, DeviceCost) for c in cost_list):
            raise TypeError("`cost` must be a DeviceCost or a sequence of DeviceCosts on the MI355X path")
        nruns = len(cost_list) if nruns is None else int(nruns)
        if len(cost_list) != nruns:
            raise ValueError(f"smc_batch: {len(cost_list)} costs for nruns = {nruns}")
    if nruns < 1:
        raise ValueError("smc_batch: nruns must be >= 1")
    c0 = cost_list[0]
    for i, c in enumerate(cost_list):
        if c.id != c0.id or c.params.size != c0.params.size or c.data.size != c0.data.size:
            raise ValueError(f"smc_batch: cost {i} differs from cost 0 in its id or its params / data lengths")
    seeds = chain_seeds(seed, nruns) if seeds is None else [int(x) for x in seeds]
    if len(seeds) != nruns:
        raise ValueError(f"smc_batch: len(seeds) = {len(seeds)} != nruns = {nruns}")
    if verbose:
        raise ValueError("smc_batch: verbose=True is not supported (one log per run: info['log'])")
    if comm is not None or shard is not None:
        raise ValueError("smc_batch: comm / shard are not supported (single-GPU batches only)")
    if log_cap is not None and int(log_cap) < 0:
        raise ValueError("smc_batch: log_cap must be >= 0")
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.SmcOpts()
    lib.kabc_smc_default_opts(C.byref(o))
    o.nparticles = int(nparticles)
    o.alpha = float(alpha)
    o.mcmc_retrys = int(mcmc_retrys)
    o.mcmc_tol = float(mcmc_tol)
    o.epstol = float(epstol)
    o.r_epstol = math.nan if r_epstol is None else float(r_epstol)
    o.min_r_ess = math.nan if min_r_ess is None else float(min_r_ess)
    o.max_stretch = float(max_stretch)
    if max_iterations is not None:
        o.max_iterations = int(max_iterations)
    R, N, D = nruns, int(nparticles), len(fac)
    n_alloc = max(N, 1)
    cap = (min(4096, max(1, _SMC_BATCH_LOG_BYTES // (C.sizeof(cd.SmcIter) * R))) if log_cap is None
           else int(log_cap))
    t_host0 = time.perf_counter()
    theta = _lib.result_empty((R, n_alloc, D))
    Cst = _lib.result_empty((R, n_alloc))
    alive = np.zeros((R, n_alloc), dtype=np.uint8)
    it_dt = np.dtype({"names": ["eps", "ess", "accepted", "resampled", "flag", "mcmc_passes", "reserved"],
                      "formats": ["<f8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4"],
                      "offsets": [getattr(cd.SmcIter, f).offset for f in
                                  ("eps", "ess", "accepted", "resampled", "flag", "mcmc_passes", "reserved")],
                      "itemsize": C.sizeof(cd.SmcIter)})
    log = np.zeros((R, max(cap, 1)), dtype=it_dt)
    # the R result records, written through a uint64 view (every field is 8 bytes wide): run r's
    # arrays follow run r - 1's, so that the library copies each array once
    res = (cd.SmcResult * R)()
    w = np.frombuffer(res, dtype=np.uint64).reshape(R, C.sizeof(cd.SmcResult) // 8)
    rr = np.arange(R, dtype=np.uint64)
    col = lambda f: getattr(cd.SmcResult, f).offset // 8   # noqa: E731
    w[:, col("theta")] = np.uint64(theta.ctypes.data) + rr * np.uint64(n_alloc * D * 8)
    w[:, col("cost")] = np.uint64(Cst.ctypes.data) + rr * np.uint64(n_alloc * 8)
    w[:, col("alive")] = np.uint64(alive.ctypes.data) + rr * np.uint64(n_alloc)
    if cap > 0:
        w[:, col("iter_log")] = np.uint64(log.ctypes.data) + rr * np.uint64(cap * it_dt.itemsize)
    w[:, col("iter_log_cap")] = np.uint64(cap)
    w[:, col("iterations")] = np.uint64(2**64 - 1)   # (-1: a run that never started)
    cc_of = {}   # (one record per distinct DeviceCost: a repeated one points at the same params)
    for c in cost_list:
        if id(c) not in cc_of:
            cc_of[id(c)] = c.to_c()
    ccs = (cd.Cost * R)(*[cc_of[id(c)] for c in cost_list])
    sd = (C.c_uint64 * R)(*seeds)
    st = (C.c_int * R)()
    with ctx.interruptible():   # (a Cancelled raised inside becomes KeyboardInterrupt after Ctrl-C)
        status = lib.kabc_smc_run_batch(ctx.handle, fac.to_c(), D, ccs, R, sd, C.byref(o), res, st)
        t_host1 = time.perf_counter()
        bs = (C.c_int64 * 4)()
        lib.kabc_smc_batch_stats(bs)

        def entry(r):
            q = res[r]
            if q.iterations < 0:
                return None
            th, mask = theta[r], alive[r].view(np.bool_)
            kept = th if (q.n_alive == n_alloc and N > 0) else th[mask]
            info = _RunInfo({"iterations": q.iterations, "n_alive": q.n_alive, "cost_evals": q.cost_evals,
                             "proposals": q.proposals, "alive": mask, "theta_all": th,
                             "kernel_ms_mcmc": q.kernel_ms_mcmc, "mcmc_launches": q.mcmc_launches})
            info._log_rows = log[r, :min(q.iterations, cap)]
            return SmcResult(kept if return_array else _bundle(kept, scalar), Cst[r], q.eps, info)

        out = SmcBatchResult(entry(r) if st[r] in (0, cd.KABC_ERR_CANCELLED) else None for r in range(R))
        out.info = {"course": "grid" if bs[0] == 1 else "sequential", "launches": int(bs[1]),
                    "runs_per_launch": int(bs[2]), "nruns": R, "log_cap": cap,
                    "wall_ms": (t_host1 - t_host0) * 1e3, "status": [int(x) for x in st]}
        if status != 0:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = out
                raise
            except _lib.KabcError as e:
                e.results = out
                raise
        return out


class AbcdeResult(collections.namedtuple("AbcdeResult", ["P", "C", "reached_eps", "info"])):
    """(P, C, reached_ϵ) of src/smc.jl:428 (+ info); `.reached_ϵ` aliases `.reached_eps`."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ("reached_\u03b5", "reached_\u03f5"):
            return self.reached_eps
        raise AttributeError(name)


def _check_with_result(status, result):
    """_lib.check; a cancelled call's exception carries what the library left in the result (`.result`)"""
    if status == cd.KABC_ERR_CANCELLED:
        try:
            _lib.check(status)
        except _lib.Cancelled as e:
            e.result = result()
            raise
    _lib.check(status)


class _PopulationState:
    """What AbcdeState and PfilterState share: `theta` [N][D] as the loop holds it (NOT push_p'ed: a discrete
    prior's particles sit between integers), `cost` and `logprior` [N], integer and float scalars named by
    the subclass; `save(path)` / `load(path)` as one .npz of arrays and scalars, no pickle."""

    _INTS = ()
    _UNSIGNED = ()
    _FLOATS = ()
    _COUNTER = None    # the counter of completed generations / iterations (-1: the run that was to fill it failed)
    _CSTRUCT = None

    def __init__(self, theta, cost, logprior, **scalars):
        name = type(self).__name__
        self.theta = np.ascontiguousarray(theta, dtype=np.float64)
        if self.theta.ndim != 2:
            raise ValueError(f"{name}: theta must be [nparticles][D]")
        n = self.theta.shape[0]
        self.cost = np.ascontiguousarray(cost, dtype=np.float64).reshape(-1)
        self.logprior = np.ascontiguousarray(logprior, dtype=np.float64).reshape(-1)
        for key in ("cost", "logprior"):
            if getattr(self, key).shape[0] != n:
                raise ValueError(f"{name}: {key} has {getattr(self, key).shape[0]} entries for {n} particles")
        if set(scalars) != set(self._INTS) | set(self._FLOATS):
            raise TypeError(f"{name}: the scalars are {', '.join(self._INTS + self._FLOATS)}")
        for key in self._INTS:
            setattr(self, key, int(scalars[key]))
        for key in self._FLOATS:
            setattr(self, key, float(scalars[key]))

    nparticles = property(lambda self: self.theta.shape[0])
    D = property(lambda self: self.theta.shape[1])

    @classmethod
    def _empty(cls, n, D):
        """the state a call fills: the counter at -1 until it has"""
        scalars = {key: 0 for key in cls._INTS}
        scalars.update({key: math.nan for key in cls._FLOATS})
        scalars[cls._COUNTER] = -1
        return cls(np.empty((n, D)), np.empty(n), np.empty(n), **scalars)

    def save(self, path):
        """Write the state to `path` as one .npz (the name is used as given)."""
        arrays = {"theta": self.theta, "cost": self.cost, "logprior": self.logprior}
        for key in self._INTS:
            arrays[key] = (np.uint64 if key in self._UNSIGNED else np.int64)(getattr(self, key))
        for key in self._FLOATS:
            arrays[key] = np.float64(getattr(self, key))
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["theta"], z["cost"], z["logprior"], **{key: int(z[key]) for key in cls._INTS},
                       **{key: float(z[key]) for key in cls._FLOATS})

    def _to_c(self):
        st = self._CSTRUCT()
        st.nparticles, st.D = self.nparticles, self.D
        for key in self._INTS + self._FLOATS:
            setattr(st, key, getattr(self, key))
        st.theta = self.theta.ctypes.data_as(cd.c_double_p)
        st.cost = self.cost.ctypes.data_as(cd.c_double_p)
        st.logprior = self.logprior.ctypes.data_as(cd.c_double_p)
        return st

    def _take_scalars(self, st):
        """the scalars the library wrote into the struct; the arrays it filled in place"""
        for key in self._INTS + self._FLOATS:
            setattr(self, key, getattr(st, key))


class AbcdeState(_PopulationState):
    """What an ABCDE run holds at a generation boundary (kabc_abcde_state_t, include/kabc.h): enough to go
    on from there with `ABCDE(prior, cost, ϵ_target, resume=state, ...)`, bit for bit as if the run had never
    stopped -- given the same prior, cost, seed and options.  `generation` counts the generations whose
    moves have run (the generation counter of the random streams), `nsims` the simulations so far."""

    _INTS = ("seed", "generation", "nsims")
    _UNSIGNED = ("seed", "nsims")
    _COUNTER = "generation"
    _CSTRUCT = cd.AbcdeState


class PfilterState(_PopulationState):
    """What a pfilter run holds at an iteration boundary (kabc_pfilter_state_t, include/kabc.h): enough to go
    on from there with `pfilter(prior, cost, N, resume=state, ...)`, bit for bit as if the run had never
    stopped -- given the same prior, cost, seed and options.  `nparticles` is the effective N
    (kabc_pfilter_nparticles), `iteration` counts the completed iterations (0: the initial draw), `eps`
    and `eff` are those of the last one (Inf / NaN at iteration 0), `nreps` and `cost_evals` are totals."""

    _INTS = ("seed", "iteration", "nreps", "cost_evals")
    _UNSIGNED = ("seed", "nreps", "cost_evals")
    _FLOATS = ("eps", "eff")
    _COUNTER = "iteration"
    _CSTRUCT = cd.PfilterState


def _resume_keywords(name, state_cls, resume, nparticles, what, D, seed):
    """smc()'s rules for `nparticles` and `seed` against a state, raised before the library is touched"""
    if not isinstance(resume, state_cls):
        raise TypeError(f"{name}: resume must be a{'n' if state_cls.__name__[0] in 'AEIOU' else ''} "
                        f"{state_cls.__name__}")
    if nparticles is not None and int(nparticles) != resume.nparticles:
        raise ValueError(f"{name}: {what} = {int(nparticles)}, the state holds {resume.nparticles} particles")
    if D != resume.D:
        raise ValueError(f"{name}: length(prior) = {D}, the state's particles have {resume.D} parameters")
    return resume.nparticles, (resume.seed if seed is None else seed)


class _Default(int):
    """a keyword's documented default, told apart from the same number given by the caller: with resume= the
    state's value holds unless the caller names one"""


_ABCDE_NPARTICLES = _Default(50)


def ABCDE(prior, cost, eps_target, *, nparticles=_ABCDE_NPARTICLES, generations=20, α=0.0, alpha=None,
          parallel=False, earlystop=False, verbose=False, proposal_width=1.0, seed=None, ctx=None,
          return_array=False, return_state=False, resume=None):
    """ABCDE(prior, cost, ϵ_target; ...) -- src/smc.jl:347-430, same keywords and defaults (nparticles = 50,
    seed = 0; `alpha` is an ASCII alias of `α`; `parallel` is accepted and ignored).
    Context.cancel() or Ctrl-C stops the run at a generation boundary: Cancelled (its `.result` holds the
    population after the k generations that completed, the result of `generations = k`) or
    KeyboardInterrupt.
    `return_state=True` (kabc_abcde_run_from): info["state"] is the AbcdeState the run ended in -- also on
    Cancelled.result.  `resume=state` continues from it instead of drawing from the prior: `nparticles` and
    `seed` default to the state's; `generations` bounds the total, and info["generations_run"] and
    info["nsims"] count from the start of the run.  With the same prior, cost, seed and options the continued
    run is the uninterrupted one, bit for bit; a state that already holds `generations` generations comes
    back unchanged.
    Returns (P, C, reached_ϵ) as the reference does (+ info)."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if resume is not None:
        nparticles, seed = _resume_keywords("ABCDE", AbcdeState, resume,
                                            None if nparticles is _ABCDE_NPARTICLES else nparticles, "nparticles",
                                            len(fac), seed)
    seed = 0 if seed is None else seed
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.AbcdeOpts()
    lib.kabc_abcde_default_opts(C.byref(o))
    o.nparticles, o.generations, o.eps_target = int(nparticles), int(generations), float(eps_target)
    o.alpha = float(α if alpha is None else alpha)
    o.proposal_width, o.earlystop, o.verbose, o.seed = (float(proposal_width), int(bool(earlystop)),
                                                        int(bool(verbose)), int(seed))
    N, D = max(int(nparticles), 1), len(fac)
    theta = np.empty((N, D))
    Cst = np.empty(N)
    r = cd.AbcdeResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    cc = cost.to_c()
    to = AbcdeState._empty(N, D) if return_state else None
    st_to = to._to_c() if to is not None else None
    st_from = resume._to_c() if resume is not None else None

    def result():
        info = {"generations_run": r.generations_run, "nsims": r.nsims}
        if to is not None:
            to._take_scalars(st_to)
            info["state"] = to
        return AbcdeResult(theta if return_array else _bundle(theta, scalar), Cst, bool(r.reached_eps), info)

    with ctx.interruptible():
        # (a state in or out: kabc_abcde_run_from; else kabc_abcde_run, which copies nothing more)
        if to is None and resume is None:
            status = lib.kabc_abcde_run(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r))
        else:
            status = lib.kabc_abcde_run_from(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o),
                                             C.byref(st_from) if st_from is not None else None,
                                             C.byref(st_to) if st_to is not None else None, C.byref(r))
        _check_with_result(status, result)
    return result()


class AbcdeBatchResult(list):
    """ABCDE_batch's result: one AbcdeResult per run (a list), and `.info` about the whole call."""

    info = None


def ABCDE_batch(prior, cost, eps_target, nruns=None, *, seeds=None, seed=0, nparticles=50, generations=20,
                α=0.0, alpha=None, earlystop=False, proposal_width=1.0, parallel=False, verbose=False, ctx=None,
                return_array=False):
    """Many independent ABCDE runs in one call (kabc_abcde_run_batch): run r is
    ABCDE(prior, cost_r, eps_target, seed=seeds[r], <the same keywords>), bit for bit.

    `cost` is one DeviceCost (the runs differ by their seeds only; `nruns` is required) or a sequence
    of DeviceCosts, one per dataset, with the same cost id and the same params and data lengths
    (`nruns` defaults to its length).  `seeds` defaults to chain_seeds(seed, nruns).  With
    3 <= nparticles <= 256 and length(prior) <= KABC_MAX_DIM the runs are the workgroups of ONE launch
    (info["course"] == "grid"); other shapes run one after another ("sequential").  `verbose` is
    refused; `parallel` is accepted and ignored, as ABCDE does.

    Returns a list of AbcdeResult, entry r as ABCDE returns it (its P / C are views into one
    [nruns][N][D] / [nruns][N] block); the list's `.info` holds the course, the kernel launches, the
    runs per launch, the wall time and the runs' statuses.  A failed run raises KabcError("run r: ...")
    whose `.results` is the list with None at the failed runs; Context.cancel() / Ctrl-C raise Cancelled
    whose `.result` is the list of the runs' populations after the generations they completed (None for
    runs never started)."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if isinstance(cost, DeviceCost):
        if nruns is None:
            raise ValueError("ABCDE_batch: nruns is required with a single DeviceCost")
        nruns = int(nruns)
        cost_list = [cost] * max(nruns, 0)
    else:
        cost_list = list(cost)
        if not all(isinstance(c, DeviceCost) for c in cost_list):
            raise TypeError("`cost` must be a DeviceCost or a sequence of DeviceCosts on the MI355X path")
        nruns = len(cost_list) if nruns is None else int(nruns)
        if len(cost_list) != nruns:
            raise ValueError(f"ABCDE_batch: {len(cost_list)} costs for nruns = {nruns}")
    if nruns < 1:
        raise ValueError("ABCDE_batch: nruns must be >= 1")
    c0 = cost_list[0]
    for i, c in enumerate(cost_list):
        if c.id != c0.id or c.params.size != c0.params.size or c.data.size != c0.data.size:
            raise ValueError(f"ABCDE_batch: cost {i} differs from cost 0 in its id or its params / data lengths")
    seeds = chain_seeds(seed, nruns) if seeds is None else [int(x) for x in seeds]
    if len(seeds) != nruns:
        raise ValueError(f"ABCDE_batch: len(seeds) = {len(seeds)} != nruns = {nruns}")
    if verbose:
        raise ValueError("ABCDE_batch: verbose=True is not supported")
    a = float(α if alpha is None else alpha)
    if not (0.0 <= a < 1.0):   # @assert 0<=α<1 (src/smc.jl:348), before the library runs anything
        raise ValueError("α must be in 0 <= α < 1.")
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.AbcdeOpts()
    lib.kabc_abcde_default_opts(C.byref(o))
    o.nparticles, o.generations, o.eps_target = int(nparticles), int(generations), float(eps_target)
    o.alpha = a
    o.proposal_width, o.earlystop, o.verbose = float(proposal_width), int(bool(earlystop)), 0
    R, N, D = nruns, max(int(nparticles), 1), len(fac)
    t_host0 = time.perf_counter()
    theta = _lib.result_empty((R, N, D))
    Cst = _lib.result_empty((R, N))
    # the R result records, written through a uint64 view (every field is 8 bytes wide, reached_eps and
    # reserved share one): run r's arrays follow run r - 1's, so that the library copies each array once
    res = (cd.AbcdeResult * R)()
    w = np.frombuffer(res, dtype=np.uint64).reshape(R, C.sizeof(cd.AbcdeResult) // 8)
    rr = np.arange(R, dtype=np.uint64)
    col = lambda f: getattr(cd.AbcdeResult, f).offset // 8   # noqa: E731
    w[:, col("theta")] = np.uint64(theta.ctypes.data) + rr * np.uint64(N * D * 8)
    w[:, col("cost")] = np.uint64(Cst.ctypes.data) + rr * np.uint64(N * 8)
    w[:, col("generations_run")] = np.uint64(2**64 - 1)   # (-1: a run that never started)
    cc_of = {}   # (one record per distinct DeviceCost: a repeated one points at the same params)
    for c in cost_list:
        if id(c) not in cc_of:
            cc_of[id(c)] = c.to_c()
    ccs = (cd.Cost * R)(*[cc_of[id(c)] for c in cost_list])
    sd = (C.c_uint64 * R)(*seeds)
    st = (C.c_int * R)()
    with ctx.interruptible():   # (a Cancelled raised inside becomes KeyboardInterrupt after Ctrl-C)
        status = lib.kabc_abcde_run_batch(ctx.handle, fac.to_c(), D, ccs, R, sd, C.byref(o), res, st)
        t_host1 = time.perf_counter()
        bs = (C.c_int64 * 4)()
        lib.kabc_abcde_batch_stats(bs)

        def entry(r):
            q = res[r]
            if q.generations_run < 0:
                return None
            info = {"generations_run": q.generations_run, "nsims": q.nsims}
            return AbcdeResult(theta[r] if return_array else _bundle(theta[r], scalar), Cst[r],
                               bool(q.reached_eps), info)

        out = AbcdeBatchResult(entry(r) if st[r] in (0, cd.KABC_ERR_CANCELLED) else None for r in range(R))
        out.info = {"course": "grid" if bs[0] == 1 else "sequential", "launches": int(bs[1]),
                    "runs_per_launch": int(bs[2]), "nruns": R, "wall_ms": (t_host1 - t_host0) * 1e3,
                    "status": [int(x) for x in st]}
        if status != 0:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = out
                raise
            except _lib.KabcError as e:
                e.results = out
                raise
        return out


PfilterResult = collections.namedtuple("PfilterResult", ["P", "C", "info"])


def pfilter(prior, cost, N=None, *, q=0.7, eff_tol=0.1, epstol=-math.inf, max_iters=math.inf,
            proposal_width=0.75, verbose=False, parallel=False, seed=None, ctx=None,
            return_array=False, return_state=False, resume=None):
    """pfilter(prior, cost, N; ...) -- src/smc.jl:275-340, same keywords (seed = 0; `parallel` accepted and
    ignored).
    Context.cancel() or Ctrl-C stops the run at an iteration boundary: Cancelled (its `.result` holds the
    population after the k iterations that completed, the result of `max_iters = k - 1`; k = 0: the
    initial draw) or KeyboardInterrupt.
    `return_state=True` (kabc_pfilter_run_from): info["state"] is the PfilterState the run ended in -- also
    on Cancelled.result.  `resume=state` continues from it instead of drawing from the prior: `N` and `seed`
    default to the state's, and `N`, when given, is the EFFECTIVE particle count the state holds
    (info["nparticles"]); iterations, nreps, cost_evals and `max_iters` count from the start of the run.
    With the same prior, cost, seed and options the continued run is the uninterrupted one, bit for bit.
    The stop tests are applied to the state first: a run that ended by rule stays as it is under the same
    options and goes on under a smaller `epstol` or `eff_tol` or a larger `max_iters`.
    Returns (P, C) as the reference does (+ info)."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if resume is not None:
        N, seed = _resume_keywords("pfilter", PfilterState, resume, N, "N", len(fac), seed)
    elif N is None:
        raise TypeError("pfilter: N is required (or resume=)")
    seed = 0 if seed is None else seed
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    o.nparticles, o.q, o.eff_tol, o.epstol = int(N), float(q), float(eff_tol), float(epstol)
    o.proposal_width, o.verbose, o.seed = float(proposal_width), int(bool(verbose)), int(seed)
    o.max_iters = -1 if math.isinf(max_iters) else int(math.floor(max_iters))
    D = len(fac)
    n_eff = lib.kabc_pfilter_nparticles(int(N), float(q), D)
    theta = np.empty((n_eff, D))
    Cst = np.empty(n_eff)
    r = cd.PfilterResult()
    r.theta = theta.ctypes.data_as(cd.c_double_p)
    r.cost = Cst.ctypes.data_as(cd.c_double_p)
    cc = cost.to_c()
    to = PfilterState._empty(n_eff, D) if return_state else None
    st_to = to._to_c() if to is not None else None
    st_from = resume._to_c() if resume is not None else None

    def result():
        info = {"eps": r.eps, "eff": r.eff, "iterations": r.iterations, "nreps": r.nreps,
                "cost_evals": r.cost_evals, "nparticles": n_eff}
        if to is not None:
            to._take_scalars(st_to)
            info["state"] = to
        return PfilterResult(theta if return_array else _bundle(theta, scalar),
                             Cst if return_array else Particles(Cst), info)

    with ctx.interruptible():
        # (a state in or out: kabc_pfilter_run_from; else kabc_pfilter_run, which copies nothing more)
        if to is None and resume is None:
            status = lib.kabc_pfilter_run(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o), C.byref(r))
        else:
            status = lib.kabc_pfilter_run_from(ctx.handle, fac.to_c(), D, C.byref(cc), C.byref(o),
                                               C.byref(st_from) if st_from is not None else None,
                                               C.byref(st_to) if st_to is not None else None, C.byref(r))
        _check_with_result(status, result)
    return result()


class PfilterBatchResult(list):
    """pfilter_batch's result: one PfilterResult per run (a list), and `.info` about the whole call."""

    info = None


def pfilter_batch(prior, cost, N, nruns=None, *, seeds=None, seed=0, q=0.7, eff_tol=0.1, epstol=-math.inf,
                  max_iters=math.inf, proposal_width=0.75, parallel=False, verbose=False, ctx=None,
                  return_array=False):
    """Many independent pfilter runs in one call (kabc_pfilter_run_batch): run r is
    pfilter(prior, cost_r, N, seed=seeds[r], <the same keywords>), bit for bit.

    `cost` is one DeviceCost (the runs differ by their seeds only; `nruns` is required) or a sequence
    of DeviceCosts, one per dataset, with the same cost id and the same params and data lengths
    (`nruns` defaults to its length).  `seeds` defaults to chain_seeds(seed, nruns).  With at most 256
    particles (after pfilter's own raising of N) and length(prior) <= KABC_MAX_DIM the runs are the
    workgroups of ONE launch (info["course"] == "grid"); other shapes run one after another
    ("sequential").  `verbose` is refused; `parallel` is accepted and ignored, as pfilter does.

    Returns a list of PfilterResult, entry r as pfilter returns it (its P / C are views into one
    [nruns][N_eff][D] / [nruns][N_eff] block); the list's `.info` holds the course, the kernel launches,
    the runs per launch, the wall time, the runs' statuses and the particle count.  A failed run raises
    KabcError("run r: ...") whose `.results` is the list with None at the failed runs; Context.cancel() /
    Ctrl-C raise Cancelled whose `.result` is the list of the runs as they ended -- finished, stopped
    after k >= 1 iterations (that of the same run with max_iters = k - 1), or None for runs never
    started."""
    fac = as_factored(prior)
    scalar = isinstance(prior, UnivariateDistribution)
    if isinstance(cost, DeviceCost):
        if nruns is None:
            raise ValueError("pfilter_batch: nruns is required with a single DeviceCost")
        nruns = int(nruns)
        cost_list = [cost] * max(nruns, 0)
    else:
        cost_list = list(cost)
        if not all(isinstance(c, DeviceCost) for c in cost_list):
            raise TypeError("`cost` must be a DeviceCost or a sequence of DeviceCosts on the MI355X path")
        nruns = len(cost_list) if nruns is None else int(nruns)
        if len(cost_list) != nruns:
            raise ValueError(f"pfilter_batch: {len(cost_list)} costs for nruns = {nruns}")
    if nruns < 1:
        raise ValueError("pfilter_batch: nruns must be >= 1")
    c0 = cost_list[0]
    for i, c in enumerate(cost_list):
        if c.id != c0.id or c.params.size != c0.params.size or c.data.size != c0.data.size:
            raise ValueError(f"pfilter_batch: cost {i} differs from cost 0 in its id or its params / data lengths")
    seeds = chain_seeds(seed, nruns) if seeds is None else [int(x) for x in seeds]
    if len(seeds) != nruns:
        raise ValueError(f"pfilter_batch: len(seeds) = {len(seeds)} != nruns = {nruns}")
    if verbose:
        raise ValueError("pfilter_batch: verbose=True is not supported")
    if not (0.0 < float(q) <= 1.0) or int(N) < 1:   # (the library's own check, before it runs anything)
        raise ValueError("pfilter needs 0 < q <= 1 and N >= 1")
    lib = _lib.load()
    ctx = ctx or _lib.default_context()
    o = cd.PfilterOpts()
    lib.kabc_pfilter_default_opts(C.byref(o))
    o.nparticles, o.q, o.eff_tol, o.epstol = int(N), float(q), float(eff_tol), float(epstol)
    o.proposal_width, o.verbose = float(proposal_width), 0
    o.max_iters = -1 if math.isinf(max_iters) else int(math.floor(max_iters))
    R, D = nruns, len(fac)
    n_eff = lib.kabc_pfilter_nparticles(int(N), float(q), D)
    t_host0 = time.perf_counter()
    theta = _lib.result_empty((R, n_eff, D))
    Cst = _lib.result_empty((R, n_eff))
    # the R result records, written through a uint64 view (every field is 8 bytes wide): run r's arrays
    # follow run r - 1's, so that the library copies each array once
    res = (cd.PfilterResult * R)()
    w = np.frombuffer(res, dtype=np.uint64).reshape(R, C.sizeof(cd.PfilterResult) // 8)
    rr = np.arange(R, dtype=np.uint64)
    col = lambda f: getattr(cd.PfilterResult, f).offset // 8   # noqa: E731
    w[:, col("theta")] = np.uint64(theta.ctypes.data) + rr * np.uint64(n_eff * D * 8)
    w[:, col("cost")] = np.uint64(Cst.ctypes.data) + rr * np.uint64(n_eff * 8)
    w[:, col("iterations")] = np.uint64(2**64 - 1)   # (-1: a run that never started)
    cc_of = {}   # (one record per distinct DeviceCost: a repeated one points at the same params)
    for c in cost_list:
        if id(c) not in cc_of:
            cc_of[id(c)] = c.to_c()
    ccs = (cd.Cost * R)(*[cc_of[id(c)] for c in cost_list])
    sd = (C.c_uint64 * R)(*seeds)
    st = (C.c_int * R)()
    with ctx.interruptible():   # (a Cancelled raised inside becomes KeyboardInterrupt after Ctrl-C)
        status = lib.kabc_pfilter_run_batch(ctx.handle, fac.to_c(), D, ccs, R, sd, C.byref(o), res, st)
        t_host1 = time.perf_counter()
        bs = (C.c_int64 * 4)()
        lib.kabc_pfilter_batch_stats(bs)

        def entry(r):
            x = res[r]
            if x.iterations < 0:
                return None
            info = {"eps": x.eps, "eff": x.eff, "iterations": x.iterations, "nreps": x.nreps,
                    "cost_evals": x.cost_evals, "nparticles": n_eff}
            return PfilterResult(theta[r] if return_array else _bundle(theta[r], scalar),
                                 Cst[r] if return_array else Particles(Cst[r]), info)

        out = PfilterBatchResult(entry(r) if st[r] in (0, cd.KABC_ERR_CANCELLED) else None for r in range(R))
        out.info = {"course": "grid" if bs[0] == 1 else "sequential", "launches": int(bs[1]),
                    "runs_per_launch": int(bs[2]), "nruns": R, "wall_ms": (t_host1 - t_host0) * 1e3,
                    "status": [int(x) for x in st], "nparticles": n_eff}
        if status != 0:
            try:
                _lib.check(status)
            except _lib.Cancelled as e:
                e.result = out
                raise
            except _lib.KabcError as e:
                e.results = out
                raise
        return out
