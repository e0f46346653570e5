"""DeviceCost: the `cost` argument of ApproxKernelizedPosterior / ApproxPosterior /
smc on the device path.  The reference takes an arbitrary Julia closure
(src/types.jl:42,55; src/smc.jl:94); a gfx950 kernel cannot call one, so a
cost is an id + parameter/data arrays whose formula lives in
include/kabc_costs.h (evaluated by the HIP kernels)."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import threading

import numpy as np

from . import _cdefs as cd


class DeviceCost:
    def __init__(self, cost_id, params=(), data=(), name=None, dim=None):
        self.id = int(cost_id)
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).ravel())
        self.data = np.ascontiguousarray(np.asarray(data, dtype=np.float64).ravel())
        self.name = name or f"cost{cost_id}"
        self.dim = dim   # length(θ) when the cost takes exactly one (checked by evaluate / prior_predictive)

    def to_c(self):
        c = cd.Cost()
        c.id = self.id
        c.nparams = self.params.size
        c.params = self.params.ctypes.data_as(cd.c_double_p) if self.params.size else None
        c.ndata = self.data.size
        c.data = self.data.ctypes.data_as(cd.c_double_p) if self.data.size else None
        return c

    def evaluate(self, theta, nrep=None, seed=0, first_row=0, ctx=None):
        """The cost at given parameter rows, on the GPU (kabc_cost_eval, include/kabc.h): what the
        reference writes `cost(θ)` / `cost.(res.P)` (its cost is a closure, src/types.jl:42,55).

        `theta`: one row [D] or rows [n][D], evaluated as given (no prior, no push_p).  Returns [n]
        (`nrep=None`: one replicate) or [n][nrep]; a single row drops the leading axis, so
        `cost.evaluate(x)` of one point is a float.  Replicate j of row i draws from the stream
        (seed, walker = first_row + i, t = j, DOM_EVAL_COST): the value depends on
        (seed, first_row + i, j, row, cost) alone, so `evaluate(theta)[a:b]` equals
        `evaluate(theta[a:b], first_row=a)`.  Context.cancel() / Ctrl-C: Cancelled /
        KeyboardInterrupt."""
        from . import _lib
        a = np.asarray(theta, dtype=np.float64)
        if a.ndim not in (1, 2) or a.shape[-1] < 1:
            raise ValueError("theta is one row [D] or rows [n][D], D >= 1")
        single = a.ndim == 1
        rows = np.ascontiguousarray(a.reshape(-1, a.shape[-1]))
        n, D = rows.shape
        check_eval_args(self, D, nrep, first_row, n)
        R = 1 if nrep is None else int(nrep)
        out = _lib.result_empty((n, R))
        ctx = ctx or _lib.default_context()
        cc = self.to_c()
        with ctx.interruptible():
            _lib.check(_lib.load().kabc_cost_eval(ctx.handle, C.byref(cc), D, n, rows.ctypes.data_as(cd.c_double_p),
                                                  R, int(seed), int(first_row), out.ctypes.data_as(cd.c_double_p)))
        if nrep is None:
            out = out[:, 0]
        if single:
            return float(out[0]) if nrep is None else out[0]
        return out

    __call__ = evaluate

    def __repr__(self):
        return f"DeviceCost({self.name})"


def check_eval_args(cost, D, nrep, first_row, n):
    """the refusals of DeviceCost.evaluate / prior_predictive that need no library"""
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if not 1 <= D <= cd.KABC_MAX_DIM_DYN:
        raise ValueError(f"length(θ) = {D} outside 1..{cd.KABC_MAX_DIM_DYN}")
    if cost.dim is not None and int(cost.dim) != D:
        raise ValueError(f"{cost!r} takes rows of {int(cost.dim)} parameters, got {D}")
    if nrep is not None and int(nrep) < 1:
        raise ValueError("nrep must be >= 1")
    check_rows(n, first_row)


def check_rows(n, first_row, what="n"):
    """`n` rows of the stream from `first_row`: a row is addressed by a 32-bit walker word (shared by
    DeviceCost.evaluate, prior_predictive and abc_reject; `what` names the count in the message)"""
    if int(n) < 0:
        raise ValueError(f"{what} must be >= 0")
    if int(first_row) < 0 or int(first_row) + int(n) > 1 << 32:
        raise ValueError(f"first_row must be >= 0 and first_row + {what} <= 2^32")


def check_reject_args(cost, D, eps, n, draws, keep, first_row):
    """the refusals of abc_reject that need no library; returns (n_accept, max_draws, keep) as
    kabc_reject_opts_t takes them (keep = 0: threshold mode; max_draws = 0: the whole stream)"""
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if not 1 <= D <= cd.KABC_MAX_DIM_DYN:
        raise ValueError(f"length(θ) = {D} outside 1..{cd.KABC_MAX_DIM_DYN}")
    if cost.dim is not None and int(cost.dim) != D:
        raise ValueError(f"{cost!r} takes rows of {int(cost.dim)} parameters, got {D}")
    if keep is not None:
        if eps is not None or n is not None:
            raise ValueError("give either (eps, n) or (draws, keep), not both")
        if draws is None:
            raise ValueError("keep needs draws: the best `keep` of `draws` rows")
        if int(keep) < 1:
            raise ValueError("keep must be >= 1")
        if int(draws) < int(keep):
            raise ValueError("draws must be >= keep")
    else:
        if eps is None or n is None:
            raise ValueError("give either (eps, n) or (draws, keep)")
        if math.isnan(float(eps)):
            raise ValueError("eps is NaN")
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        if draws is not None and int(draws) < 1:
            raise ValueError("draws must be >= 1")
    check_rows(0 if draws is None else draws, first_row, "draws")
    return (0 if keep is not None else int(n)), (0 if draws is None else int(draws)), (0 if keep is None else int(keep))


def check_pmc_args(cost, prior, nparticles, eps, q, eps0, eps_target, generations, kernel, scale, max_draws, min_rate):
    """the refusals of abc_pmc that need no library; returns (N, eps array or None, q, generations, kernel id,
    max_draws) as kabc_pmc_opts_t takes them (eps None: the adaptive schedule)"""
    D = len(prior)
    if not isinstance(cost, DeviceCost):
        raise TypeError("`cost` must be a DeviceCost on the MI355X path")
    if not 1 <= D <= cd.KABC_MAX_DIM:
        raise ValueError(f"length(θ) = {D} outside 1..{cd.KABC_MAX_DIM}")
    if cost.dim is not None and int(cost.dim) != D:
        raise ValueError(f"{cost!r} takes rows of {int(cost.dim)} parameters, got {D}")
    if any(getattr(c, "discrete", False) for c in prior.p):
        raise ValueError("abc_pmc needs a continuous prior: a Gaussian proposal density is not a pmf")
    N = int(nparticles)
    if not D + 2 <= N <= cd.KABC_PMC_MAX_PARTICLES:
        raise ValueError(f"nparticles = {N} outside D + 2 = {D + 2} .. 2^20")
    if kernel not in ("full", "diag"):
        raise ValueError('kernel must be "full" or "diag"')
    if not float(scale) > 0.0:
        raise ValueError("scale must be > 0")
    if math.isnan(float(min_rate)):
        raise ValueError("min_rate is NaN")
    if eps is not None:
        if q is not None:
            raise ValueError("give either eps (an explicit schedule) or q (the adaptive one), not both")
        eps = np.ascontiguousarray(np.asarray(eps, dtype=np.float64).ravel())
        if eps.size < 1 or np.isnan(eps).any():
            raise ValueError("eps is empty or holds a NaN")
        if generations is not None and int(generations) != eps.size:
            raise ValueError("generations must be len(eps) with an explicit schedule")
        G = eps.size
    else:
        q = 0.5 if q is None else float(q)
        if not 0.0 < q < 1.0:
            raise ValueError("q outside (0, 1)")
        if math.isnan(float(eps0)) or math.isnan(float(eps_target)):
            raise ValueError("eps0 / eps_target is NaN")
        G = 20 if generations is None else int(generations)
    if not 1 <= G < 1 << 24:
        raise ValueError("generations outside 1 .. 2^24 - 1")
    M = min(1 << 32, 10_000 * N) if max_draws is None else int(max_draws)
    if not N <= M <= 1 << 32:
        raise ValueError("max_draws outside nparticles .. 2^32")
    return N, eps, q, G, (cd.PMC_KERNEL_DIAG if kernel == "diag" else cd.PMC_KERNEL_FULL), M


def check_reject_batch_args(costs, D, eps, n, nruns, seeds, draws, keep, first_row):
    """the refusals of abc_reject_batch that need no library; returns (cost_list, seeds or None, eps_list or
    None, n_accept, max_draws, keep): seeds None = one seed for every run, eps_list None = keep mode"""
    if isinstance(costs, DeviceCost):
        if nruns is None and seeds is None:
            raise ValueError("abc_reject_batch: nruns or seeds is required with a single DeviceCost")
        nruns = len(seeds) if nruns is None else int(nruns)
        cost_list = [costs] * max(nruns, 0)
    else:
        cost_list = list(costs)
        if not all(isinstance(c, DeviceCost) for c in cost_list):
            raise TypeError("`costs` must be a DeviceCost or a sequence of DeviceCosts on the MI355X path")
        nruns = len(cost_list) if nruns is None else int(nruns)
        if len(cost_list) != nruns:
            raise ValueError(f"abc_reject_batch: {len(cost_list)} costs for nruns = {nruns}")
    if not 1 <= nruns <= 65535:
        raise ValueError(f"abc_reject_batch: nruns = {nruns} is outside 1..65535")
    c0 = cost_list[0]
    for i, c in enumerate(cost_list):
        if c.id != c0.id or c.params.size != c0.params.size or c.data.size != c0.data.size:
            raise ValueError(f"abc_reject_batch: cost {i} differs from cost 0 in its id or its params / data lengths")
    if seeds is not None:
        seeds = [int(x) for x in seeds]
        if len(seeds) != nruns:
            raise ValueError(f"abc_reject_batch: len(seeds) = {len(seeds)} != nruns = {nruns}")
    eps_list = None
    if keep is None and eps is not None:
        eps_list = [float(x) for x in eps] if np.ndim(eps) else [float(eps)] * nruns
        if len(eps_list) != nruns:
            raise ValueError(f"abc_reject_batch: len(eps) = {len(eps_list)} != nruns = {nruns}")
        for r, e in enumerate(eps_list):
            if math.isnan(e):
                raise ValueError(f"abc_reject_batch: eps of run {r} is NaN")
    n_accept, max_draws, k = check_reject_args(c0, D, None if eps is None else (eps_list[0] if eps_list else eps),
                                               n, draws, keep, first_row)
    return cost_list, seeds, eps_list, n_accept, max_draws, k


def GaussDist(center):
    """‖x − c‖₂"""
    return DeviceCost(cd.COST_GAUSS_DIST, params=center, name="gauss_dist")


def Rosenbrock():
    """sqrt(Σ 100(x[k+1]−x[k]²)² + (1−x[k])²) (configs C3, C5)"""
    return DeviceCost(cd.COST_ROSENBROCK, name="rosenbrock")


def HierGaussSim(ybar_obs):
    """θ = (m, s, z₁..z_G): ȳ_g = m + s z_g + randn/√8, cost = RMS(ȳ − ȳ_obs) (config C4)"""
    return DeviceCost(cd.COST_HIER_GAUSS_SIM, data=ybar_obs, name="hier_gauss_sim")


def NormalMeanStdSim(n, mean_obs, std_obs):
    """README.md:43-49: simulate n draws N(μ,σ); hypot(mean−mean_obs, 50(std−std_obs))"""
    return DeviceCost(cd.COST_NORMAL_MEANSTD_SIM, params=[n, mean_obs, std_obs],
                      name="normal_meanstd_sim", dim=2)


def DiracSq(target=1.5):
    """test/runtests.jl:79-80: |μ²+1 − target|"""
    return DeviceCost(cd.COST_DIRAC_SQ, params=[target], name="dirac_sq", dim=1)


def AbsDiff(target):
    """test/runtests.jl:178: |x − target|"""
    return DeviceCost(cd.COST_ABS_DIFF, params=[target], name="abs_diff", dim=1)


def NormShell(target):
    """test/runtests.jl:186: |‖x‖₂ − target|"""
    return DeviceCost(cd.COST_NORM_SHELL, params=[target], name="norm_shell")


def NoisyQuadDU(target=5.5):
    """test/runtests.jl:108-109: |(n²+du)(n+0.01·randn) − target|"""
    return DeviceCost(cd.COST_NOISY_QUAD_DU, params=[target], name="noisy_quad_du", dim=2)


def Mixture(target=0.0):
    """test/runtests.jl:145-146: |μ + rand((0.1·randn, randn)) − target|"""
    return DeviceCost(cd.COST_MIXTURE, params=[target], name="mixture", dim=1)


def NoisyBanana(p_inf=0.0):
    """test/runtests.jl:242,248: 50(x+0.01z₁−y²)² + (y−1+0.01z₂)², +Inf with prob p_inf"""
    return DeviceCost(cd.COST_NOISY_BANANA, params=[p_inf], name="noisy_banana", dim=2)


def WienerRms(tdata):
    """test/runtests.jl:116-126: mean |sqrt(μ²t²+σ²t)·(0.95+0.1·rand) − tdata_t|"""
    return DeviceCost(cd.COST_WIENER_RMS, data=tdata, name="wiener_rms", dim=2)


# ---- user costs compiled at run time -------------------------------------------
_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
_CSRC = os.path.join(_HERE, "csrc")
# KABC_PLUGIN_DIR: a user cache directory (read-only installs)
_PLUGIN_DIR = os.environ.get("KABC_PLUGIN_DIR") or os.path.join(_HERE, "lib", "plugins")
_registered = {}

USER_COST_SIGNATURE = (
    "KABC_HD double kabc_user_cost(const double* x, int D, const double* params,\n"
    "                              const double* data, int64_t ndata, kabc_cost_rng_t* rng)")


_PK_BITS = {"kernelized": 1, "threshold": 2, "common": 4}


def _plugin_source(source, dims, posteriors=None):
    cond = " || ".join(f"(D) == {int(d)}" for d in dims)
    mask = 7 if not posteriors else sum({_PK_BITS[p] for p in posteriors})
    return (f"// generated by kissabc_jl_amd.costs.UserCost\n"
            f"#define KABC_USER_DIM_OK(D) ({cond})\n"
            f"#define KABC_USER_PK_MASK {mask}\n"
            f"#include <hip/hip_runtime.h>\n"
            f'#include "kabc_philox.h"\n'
            f"{source}\n"
            f"#define KABC_USER_COST_DEFINED 1\n"
            f'#include "user_plugin.inc"\n')


def _toolchain_fingerprint():
    """Hash of every header a plugin is compiled against: a cached plugin built from
    older kernels / argument structs must never be loaded by a newer library."""
    h = hashlib.sha1()
    for d in (_INCLUDE, _CSRC):
        for fn in sorted(os.listdir(d)):
            if fn.endswith((".h", ".hpp", ".inc")):
                with open(os.path.join(d, fn), "rb") as f:
                    h.update(fn.encode() + b"\0" + f.read())
    return h.hexdigest()


def build_user_plugin(source, dims, hipcc=None, posteriors=None):
    """hipcc --offload-arch=gfx950 the snippet + csrc/user_plugin.inc into a shared
    library (cached by content hash); returns its path."""
    dims = sorted({int(d) for d in dims})
    if not dims or min(dims) < 1 or max(dims) > cd.KABC_MAX_DIM_DYN:
        raise ValueError(f"dims must lie in 1..{cd.KABC_MAX_DIM_DYN}")
    text = _plugin_source(source, dims, posteriors)
    tag = hashlib.sha1((text + _toolchain_fingerprint()).encode()).hexdigest()[:16]
    os.makedirs(_PLUGIN_DIR, exist_ok=True)
    so = os.path.join(_PLUGIN_DIR, f"libkabc_user_{tag}.so")
    if not os.path.exists(so):
        # unique scratch names: several processes (torchrun ranks) may hit a cold cache with
        # the same snippet at once; whoever finishes first publishes, the others discard
        uniq = f"{os.getpid()}_{threading.get_ident()}"
        src = os.path.join(_PLUGIN_DIR, f"user_{tag}_{uniq}.hip")
        tmp = f"{so}.{uniq}.tmp"
        with open(src, "w") as f:
            f.write(text)
        cmd = [hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC",
               "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-I", _INCLUDE,
               "-I", _CSRC, "-shared", "-o", tmp, src]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("user cost failed to compile:\n" + r.stderr[-4000:])
            if os.path.exists(so):
                os.remove(tmp)
            else:
                os.replace(tmp, so)
        finally:
            for f in (src, tmp):
                try:
                    os.remove(f)
                except OSError:
                    pass
    return so


def UserCost(source, dims, params=(), data=(), name="user", posteriors=None):
    """A DeviceCost from a C snippet -- the device-path counterpart of passing an
    arbitrary closure as `cost` (src/types.jl:42,55; src/smc.jl:94).

    `source` must define

        KABC_HD double kabc_user_cost(const double* x, int D, const double* params,
                                      const double* data, int64_t ndata, kabc_cost_rng_t* rng)

    (x is the push_p'ed parameter vector; kabc_math.h / kabc_philox.h are available:
    kabc_sqrt, kabc_log, kabc_exp, kabc_cost_rng_normal2(rng, &z0, &z1), ...).
    `dims` lists the values of length(prior) to build kernels for; `posteriors` optionally
    narrows the AIS kernels to the posterior kinds the cost will be used with
    ("kernelized" = ApproxKernelizedPosterior, "threshold" = ApproxPosterior, "common" =
    CommonLogDensity; smc/ABCDE/pfilter are always available).

    The snippet is compiled in process by hipRTC (kabc_compile_cost_plugin, include/kabc.h): it
    is checked at once, and each kernel family is compiled when a model first uses it (1-5 s,
    once per process; beyond KABC_MAX_DIM parameters the run-time-dimension kernels).
    KABC_USER_PLUGIN=hipcc selects the older form instead: a plugin .so built by hipcc with every
    family and dimension (15-40 s the first time, cached on disk)."""
    from . import _lib
    dl = sorted({int(d) for d in dims})
    use_hipcc = os.environ.get("KABC_USER_PLUGIN", "hiprtc") == "hipcc"
    if use_hipcc:
        # a plugin .so prebuilt by hipcc: every family and dimension at once (15-40 s, cached on disk)
        so = build_user_plugin(source, dims, posteriors=posteriors)
        cid = _registered.get(so)
        if cid is None:
            out = C.c_int32()
            _lib.check(_lib.load().kabc_register_cost_plugin(so.encode(), C.byref(out)))
            cid = _registered[so] = out.value
    else:
        # default: compiled in process by hipRTC (kabc_compile_cost_plugin) -- the snippet is
        # checked now, each kernel family is compiled at its first use (1-5 s)
        mask = 7 if not posteriors else sum({_PK_BITS[p] for p in posteriors})
        key = ("rtc", source, tuple(dl), mask)
        cid = _registered.get(key)
        if cid is None:
            out = C.c_int32()
            arr = (C.c_int32 * len(dl))(*dl)
            _lib.check(_lib.load().kabc_compile_cost_plugin(source.encode(), arr, len(dl), mask,
                                                            C.byref(out)))
            cid = _registered[key] = out.value
    c = DeviceCost(cid, params=params, data=data, name=name)
    c.source = source
    c.dims = tuple(sorted({int(d) for d in dims}))
    return c
