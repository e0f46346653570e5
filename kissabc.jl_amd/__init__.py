"""kissabc.jl_amd -- MI355X (gfx950) walker-update path of KissABC behind the
reference's own user surface (see include/kabc.h for the C ABI it sits on).

Import name: `kissabc_jl_amd` (the directory name has a dot; the repo-root
module kissabc_jl_amd.py registers this package under that name).
"""
from . import costs
from ._cdefs import KABC_MAX_DIM
from ._lib import Cancelled, Context, KabcError, LIB_PATH, default_context
from .api import (ABCDE, ABCDE_batch, AIS, AisEnsemble, ApproxKernelizedPosterior, ApproxPosterior, CommonLogDensity,
                  MCMCThreads, PmcResult, abc_pmc, abc_reject, abc_reject_batch, compile_model, pfilter, pfilter_batch, prior_predictive, set_specialize,
                  AbcdeState, ChainSummaries, Particles, PfilterState, PosteriorSummary, SmcState, sample, sample_batch, smc, smc_batch)
from . import comm
from .comm import Comm, EnsembleGroup
from .costs import DeviceCost
from .derived import Derived
from .distributions import (Ar1Normal, Beta, Dirichlet, DiscreteUniform, Exponential, Factored, Gamma, InitFromSnippet,
                            LogNormal, MultivariateNormal, MvNormal, NegativeBinomial, Normal, Product,
                            Laplace, Poisson, Truncated, TruncatedGamma, TruncatedNormal, Uniform, UserInit,
                            UserMvPrior, UserPrior, truncated)

__all__ = [
    "ABCDE", "ABCDE_batch", "AIS", "AisEnsemble", "ApproxKernelizedPosterior", "ApproxPosterior", "CommonLogDensity",
    "MCMCThreads", "PmcResult", "abc_pmc", "abc_reject", "abc_reject_batch", "pfilter", "pfilter_batch", "prior_predictive",
    "AbcdeState", "ChainSummaries", "Particles", "PosteriorSummary", "PfilterState", "SmcState", "sample", "sample_batch", "smc", "smc_batch", "DeviceCost", "Derived", "costs", "Factored", "Uniform", "Normal",
    "Truncated", "truncated", "TruncatedNormal", "Beta", "DiscreteUniform", "NegativeBinomial",
    "Exponential", "Gamma", "LogNormal", "Product", "MvNormal", "MultivariateNormal", "Context", "KabcError", "Cancelled", "default_context", "LIB_PATH",
    "KABC_MAX_DIM", "comm", "Comm", "EnsembleGroup", "UserInit", "InitFromSnippet",
    "UserPrior", "UserMvPrior", "Dirichlet", "Ar1Normal", "Poisson", "Laplace", "TruncatedGamma", "compile_model", "set_specialize",
]
