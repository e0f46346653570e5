"""The cases of tests/test_gpu_poisoned_memory.py, and the child process that runs one family of them.

    python tests/poison_child.py <family> <out.npz>

KABC_POISON_ALLOC is read once per process (csrc/host_common.hpp), so a poisoned run needs a process of its own:
the child runs every case of one family on the device and stores every result array and scalar, the driver or
course each case took, and the bytes kabc_poison_probe read back.  It asserts nothing: a case that raises is
stored as its error text, and the parent -- which builds every expectation from the CPU oracle with the `orc`
side of the same Case -- fails on it.

A Case is (name, env, dev, orc): `env` are the per-call knobs the case runs under (every knob the library reads
is read per call, except KABC_POISON_ALLOC and KABC_POOL_MB: one child per family is enough), dev(k) and
orc(k, o) return {key: array} with the same keys; dev adds "driver" / "course" entries (strings), which the
parent compares with EXPECTED_COURSES, not with the oracle."""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_BYTES = 3 * 4096 + 5
SEEDS3 = [1, 977, 2 ** 40 + 3]
KNOBS = ("KABC_AIS_SMALL", "KABC_SMC_LOOP", "KABC_SMC_SMALL", "KABC_SMC_SPEC_SELECT", "KABC_PF_PASSES", "KABC_PF_SMALL",
         "KABC_ABCDE_RANK", "KABC_ABCDE_SMALL", "KABC_REJECT_COURSE", "KABC_REJECT_CAPACITY", "KABC_PREBUILT_CLASS",
         "KABC_DYN_LDS_WAVES", "KABC_DSEL2_G", "KABC_DSEL2_DECIDE_G", "KABC_AUX_KIB", "KABC_PF_BATCH", "KABC_EVAL_ROWS",
         "KABC_REJECT_BATCH", "KABC_REJECT_BATCH_COURSE", "KABC_REJECT_BATCH_COMPACT", "KABC_USER_PLUGIN")
DEVICE_FAULT_STATUS = 3      # the child's exit status after a device / HIP error: nothing more runs on the GPU


@contextlib.contextmanager
def knobs(env):
    """the environment of one case: every knob unset except the case's own"""
    old = {v: os.environ.pop(v, None) for v in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for v in KNOBS:
            os.environ.pop(v, None)
            if old[v] is not None:
                os.environ[v] = old[v]


class Case:
    def __init__(self, name, env, dev, orc):
        self.name, self.env, self.dev, self.orc = name, env, dev, orc


# ---- models (those of the parity tests) ------------------------------------------------------------------------
def n2_prior(k):
    return k.Factored(k.Normal(0, 5), k.Normal(0, 5))


def n2_model(k):          # tests/test_gpu_ais_small.py _n2: D = 2, GaussDist, kernelized
    return k.ApproxKernelizedPosterior(n2_prior(k), k.costs.GaussDist([1.0, -0.5]), 0.1)


def readme_prior(k):
    return k.Factored(k.Uniform(1, 3), k.Truncated(k.Normal(0, 0.1), 0, 100))


def d20_model(k, centre=0.0):   # tests/test_gpu_ais_dyn_small.py _d20
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Normal(0, 3)] * 20), k.costs.GaussDist(np.full(20, centre)), 1.0)


def d128_model(k):        # tests/test_gpu_ais_dyn_small.py gauss_d128
    return k.ApproxPosterior(k.Product([k.Uniform(-2, 2)] * 128), k.costs.GaussDist(np.zeros(128)), 12.0)


def d34_model(k):         # tests/test_gpu_ais_dyn_small.py hier_d34_mixed
    rng = np.random.default_rng(4)
    rng.normal(size=40)   # (the draws _models makes before this model's)
    return k.ApproxKernelizedPosterior(
        k.Factored(k.Normal(0, 5), k.Uniform(0, 5), *[k.Normal(0, 1)] * 30, k.Gamma(2.0, 1.0), k.DiscreteUniform(-3, 3)),
        k.costs.HierGaussSim(rng.normal(size=32)), 1.0)


def mv3_prior(k):         # tests/test_gpu_mvnormal.py _mv: a full covariance (its table is a working buffer too)
    rng = np.random.default_rng(103)
    A = rng.normal(size=(3, 3))
    return k.MvNormal(rng.normal(size=3), A @ A.T + 0.4 * np.eye(3))


def du_prior(k):          # a discrete-uniform prior: ties among the costs
    return k.Factored(k.DiscreteUniform(-20, 20), k.DiscreteUniform(-20, 20))


# ---- packing: the same keys from the device and from the oracle ------------------------------------------------
def _stats(st):
    return np.array([st["proposals"], st["cost_evals"], st["accepted"]], dtype=np.uint64)


def _debug_rows(rec, N):
    """the oracle's debug records in the device's form: partner ids as rows of the complementary half"""
    n0 = (N + 1) // 2
    ro = np.array(rec, dtype=np.int64)[..., :6].copy()
    ro[:n0, :, 2:5] = np.where(ro[:n0, :, 2:5] >= 0, ro[:n0, :, 2:5] - n0, -1)
    return ro


def _ais_pack(e, N, gens, nt, debug, is_orc):
    out = {}
    x, lp, ll, _ = e.state()
    out["init_x"], out["init_lp"], out["init_ll"] = x.copy(), lp.copy(), ll.copy()
    if debug:
        if is_orc:
            tr, rec = e.generations_sync(1, nt, trace=True)
            out["debug"] = _debug_rows(rec[0], N)
        else:
            e.set_debug(nt)
            tr = e.advance(1, nt, collect=True)
            out["debug"] = e.get_debug(nt).astype(np.int64)[..., :6]
            e.set_debug(0)
        out["trace_debug"] = np.array(tr)
    out["trace"] = np.array(e.generations_sync(gens, nt) if is_orc else e.advance(gens, nt, collect=True))
    x, lp, ll, t = e.state()
    out.update(x=x, lp=lp, ll=ll, t=np.uint64(t), stats=_stats(e.stats()))
    return out


def ais_case(name, make, N, seed, gens, nt, env, debug=False, resume=False):
    def dev(k):
        e = k.AisEnsemble(make(k), N, seed=seed).init()
        out = _ais_pack(e, N, gens, nt, debug, False)
        out["driver"] = e.driver
        if resume:   # AISState round trip into a second handle, which then goes on
            b = k.AisEnsemble(make(k), N, seed=seed)
            b.set_state(out["x"], out["lp"], out["ll"], int(out["t"]))
            out["driver_resumed"] = b.driver
            out["trace_resumed"] = np.array(b.advance(2, nt, collect=True))
            out["x_resumed"] = b.state()[0]
            b.close()
        e.close()
        return out

    def orc(k, o):
        e = o.OracleAIS(make(k), N, seed=seed).init()
        out = _ais_pack(e, N, gens, nt, debug, True)
        if resume:
            out["trace_resumed"] = np.array(e.generations_sync(2, nt))
            out["x_resumed"] = e.state()[0]
        return out
    return Case(name, env, dev, orc)


def chains_case(name, make, costs, N, seeds, gens, nt, env):
    """per-chain seeds and costs on one handle: chain c is OracleAIS on (costs[c], seeds[c])"""
    def dev(k):
        cs = costs(k)
        e = k.AisEnsemble(make(k, 0), N, seeds=seeds, costs=cs).init()
        tr = np.array(e.advance(gens, nt, collect=True))          # [gen][chain][N][D]
        st = e.state()
        out = {"driver": e.driver, "trace": tr.transpose(1, 0, 2, 3).copy(), "x": st[0], "lp": st[1], "ll": st[2]}
        e.close()
        return out

    def orc(k, o):
        tr, xs, lps, lls = [], [], [], []
        for c, sd in enumerate(seeds):
            e = o.OracleAIS(make(k, c), N, seed=sd).init()
            tr.append(e.generations_sync(gens, nt))
            x, lp, ll, _ = e.state()
            xs.append(x), lps.append(lp), lls.append(ll)
        return {"trace": np.array(tr), "x": np.array(xs), "lp": np.array(lps), "ll": np.array(lls)}
    return Case(name, env, dev, orc)


def _log_rows(log):
    return np.array([[np.float64(it["eps"]).view(np.uint64), it["ess"], it["accepted"], it["resampled"], it["flag"]]
                     for it in log], dtype=np.uint64).reshape(-1, 5)


def _smc_dev(r):
    i = r.info
    return {"theta_all": np.array(i["theta_all"]), "C": np.array(r.C), "alive": np.array(i["alive"], dtype=np.uint8),
            "eps": np.float64(r.eps), "log": _log_rows(i["log"]),
            "counts": np.array([i["iterations"], i["cost_evals"], i["proposals"]], dtype=np.uint64)}


def _smc_orc(r):
    return {"theta_all": np.array(r["theta_all"]), "C": np.array(r["C"]), "alive": np.array(r["alive"], dtype=np.uint8),
            "eps": np.float64(r["eps"]), "log": _log_rows(r["log"]),
            "counts": np.array([r["iterations"], r["cost_evals"], r["proposals"]], dtype=np.uint64)}


def smc_course(info):
    """how kabc_smc_run drove the run, from kabc_smc_dist_stats: the one-exchange course, the kernel-per-phase
    path (host looks), or a persistent kernel (loop / one workgroup: no host look)"""
    d = info["dist"]
    if d["one_exchange_selections"] > 0:
        return "one-exchange"
    return "looked" if d["host_looks"] > 0 else "persistent"


def smc_case(name, prior, cost, kw, env, ctx_calls=None):
    def dev(k):
        r = k.smc(prior(k), cost(k), return_array=True, **kw)
        out = _smc_dev(r)
        out["course"] = smc_course(r.info)
        return out

    def orc(k, o):
        return _smc_orc(o.smc(prior(k), cost(k), **kw))
    return Case(name, env, dev, orc)


def smc_batch_case(name, prior, cost, kw, seeds, env):
    def dev(k):
        res = k.smc_batch(prior(k), cost(k), len(seeds), seeds=seeds, return_array=True, **kw)
        out = {"course": res.info["course"]}
        for r in range(len(seeds)):
            out.update({f"{key}_{r}": v for key, v in _smc_dev(res[r]).items()})
        return out

    def orc(k, o):
        out = {}
        for r, sd in enumerate(seeds):
            out.update({f"{key}_{r}": v for key, v in _smc_orc(o.smc(prior(k), cost(k), seed=sd, **kw)).items()})
        return out
    return Case(name, env, dev, orc)


def _pf_dev(r):
    i = r.info
    return {"P": np.array(r.P), "C": np.array(r.C), "eps": np.float64(i["eps"]), "eff": np.float64(i["eff"]),
            "counts": np.array([i["iterations"], i["nreps"], i["cost_evals"]], dtype=np.uint64)}


def _pf_orc(r):
    return {"P": np.array(r["P"]), "C": np.array(r["C"]), "eps": np.float64(r["eps"]), "eff": np.float64(r["eff"]),
            "counts": np.array([r["iterations"], r["nreps"], r["cost_evals"]], dtype=np.uint64)}


def pf_case(name, prior, cost, N, kw, env, seeds=None):
    def dev(k):
        if seeds is None:
            return _pf_dev(k.pfilter(prior(k), cost(k), N, seed=5, return_array=True, **kw))
        res = k.pfilter_batch(prior(k), cost(k), N, len(seeds), seeds=seeds, return_array=True, **kw)
        out = {"course": res.info["course"]}
        for r in range(len(seeds)):
            out.update({f"{key}_{r}": v for key, v in _pf_dev(res[r]).items()})
        return out

    def orc(k, o):
        if seeds is None:
            return _pf_orc(o.pfilter(prior(k), cost(k), N, seed=5, **kw))
        out = {}
        for r, sd in enumerate(seeds):
            out.update({f"{key}_{r}": v for key, v in _pf_orc(o.pfilter(prior(k), cost(k), N, seed=sd, **kw)).items()})
        return out
    return Case(name, env, dev, orc)


def _de_dev(r):
    return {"P": np.array(r.P), "C": np.array(r.C),
            "counts": np.array([int(bool(r.reached_ϵ)), r.info["generations_run"], r.info["nsims"]], dtype=np.uint64)}


def _de_orc(r):
    return {"P": np.array(r["P"]), "C": np.array(r["C"]),
            "counts": np.array([int(bool(r["reached_eps"])), r["generations_run"], r["nsims"]], dtype=np.uint64)}


def de_case(name, prior, cost, eps, kw, env, seeds=None):
    def dev(k):
        if seeds is None:
            return _de_dev(k.ABCDE(prior(k), cost(k), eps, seed=5, return_array=True, **kw))
        res = k.ABCDE_batch(prior(k), cost(k), eps, len(seeds), seeds=seeds, return_array=True, **kw)
        out = {"course": res.info["course"]}
        for r in range(len(seeds)):
            out.update({f"{key}_{r}": v for key, v in _de_dev(res[r]).items()})
        return out

    def orc(k, o):
        if seeds is None:
            return _de_orc(o.abcde(prior(k), cost(k), eps, seed=5, **kw))
        out = {}
        for r, sd in enumerate(seeds):
            out.update({f"{key}_{r}": v for key, v in _de_orc(o.abcde(prior(k), cost(k), eps, seed=sd, **kw)).items()})
        return out
    return Case(name, env, dev, orc)


def reject_case(name, prior, cost, env, eps=None, n=None, draws=None, keep=None, seed=3, first_row=7):
    def dev(k):
        if keep is not None:
            r = k.abc_reject(prior(k), cost(k), draws=draws, keep=keep, seed=seed, first_row=first_row, return_array=True)
        else:
            r = k.abc_reject(prior(k), cost(k), eps, n, draws=draws, seed=seed, first_row=first_row, return_array=True)
        return {"P": np.array(r.P), "C": np.array(r.C), "logprior": np.array(r.logprior), "eps": np.float64(r.eps),
                "index": np.array(r.info["index"], dtype=np.int64),
                "counts": np.array([r.info["draws"], int(r.info["exhausted"])], dtype=np.uint64),
                "course": r.info["course"], "launches": np.int64(r.info["launches"])}

    def orc(k, o):
        from abc_reject_oracle import oracle_reject
        P, C_, lp, e, idx, d, x = oracle_reject(o, prior(k), cost(k), eps=eps, n=n, draws=draws, keep=keep, seed=seed,
                                                first_row=first_row)
        return {"P": P, "C": C_, "logprior": lp, "eps": np.float64(e), "index": np.array(idx, dtype=np.int64),
                "counts": np.array([d, int(x)], dtype=np.uint64)}
    return Case(name, env, dev, orc)


def recycled_smc_case(name, prior, cost, kw, env, big=4096, small=2500):
    """a smaller run on the buffers a larger one left in the pool of the same context (DevBufs::alloc hands out
    any cached buffer up to twice too large); with KABC_POOL_MB=0 the same calls on fresh buffers"""
    def dev(k):
        ctx = k.Context(0)
        try:
            k.smc(prior(k), cost(k), nparticles=big, ctx=ctx, return_array=True, **kw)
            r = k.smc(prior(k), cost(k), nparticles=small, ctx=ctx, return_array=True, **kw)
        finally:
            ctx.close()
        out = _smc_dev(r)
        out["course"] = smc_course(r.info)
        return out

    def orc(k, o):
        return _smc_orc(o.smc(prior(k), cost(k), nparticles=small, **kw))
    return Case(name, env, dev, orc)


def _rej_dev(r):
    return {"P": np.array(r.P), "C": np.array(r.C), "logprior": np.array(r.logprior), "eps": np.float64(r.eps),
            "index": np.array(r.info["index"], dtype=np.int64),
            "counts": np.array([r.info["draws"], int(r.info["exhausted"])], dtype=np.uint64)}


def reject_batch_case(name, prior, costs, seeds, env, eps=None, n=None, draws=None, keep=None, first_row=7, ctx=None):
    def dev(k, ctx=None):
        if keep is not None:
            res = k.abc_reject_batch(prior(k), costs(k), seeds=seeds, draws=draws, keep=keep, first_row=first_row,
                                     return_array=True, ctx=ctx)
        else:
            res = k.abc_reject_batch(prior(k), costs(k), eps, n, seeds=seeds, draws=draws, first_row=first_row,
                                     return_array=True, ctx=ctx)
        out = {"course": res.info["course"]}
        for r in range(len(seeds)):
            out.update({f"{key}_{r}": v for key, v in _rej_dev(res[r]).items()})
        return out

    def orc(k, o):
        from abc_reject_batch_oracle import batch_tables, expected_batch
        want = expected_batch(batch_tables(o, prior(k), costs(k), draws, seeds, first_row), eps=eps, n=n, keep=keep)
        out = {}
        for r, w in enumerate(want):
            out.update({f"P_{r}": w["P"], f"C_{r}": w["C"], f"logprior_{r}": w["logprior"], f"eps_{r}": np.float64(w["eps"]),
                        f"index_{r}": np.array(w["index"], dtype=np.int64),
                        f"counts_{r}": np.array([w["draws"], int(w["exhausted"])], dtype=np.uint64)})
        return out
    return Case(name, env, dev, orc)


def _cost_table(o, cost, theta, seed, first_row, nrep):
    from kissabc_jl_amd import _cdefs as cd
    return np.array([[o.cost_eval(cost, theta[i], seed=seed, walker=first_row + i, t=j, domain=cd.DOM_EVAL_COST)
                      for j in range(nrep)] for i in range(len(theta))], dtype=np.float64)


def evaluate_case(name, cost, D, n, nrep, env, seed=3, first_row=5, user=False):
    theta = np.random.default_rng(17).normal(size=(n, D)) * 1.5

    def dev(k, ctx=None):
        return {"C": np.array(cost(k).evaluate(theta, nrep=nrep, seed=seed, first_row=first_row, ctx=ctx))}

    def orc(k, o):
        c = cost(k)
        if user:
            o.register_user_cost(c)
        return {"C": _cost_table(o, c, theta, seed, first_row, nrep)}
    return Case(name, env, dev, orc)


def predictive_case(name, prior, cost, n, env, seed=4, first_row=9):
    def dev(k, ctx=None):
        r = k.prior_predictive(prior(k), cost(k), n, seed=seed, first_row=first_row, return_array=True, ctx=ctx)
        return {"P": np.array(r.P), "C": np.array(r.C), "logprior": np.array(r.logprior),
                "launches": np.int64(r.info["launches"])}

    def orc(k, o):
        from abc_reject_oracle import oracle_table
        P, lp, C_ = oracle_table(o, prior(k), cost(k), n, seed, first_row)
        return {"P": P, "C": C_, "logprior": lp}
    return Case(name, env, dev, orc)


def priors_case(name, prior, n, env):
    x = np.random.default_rng(2).normal(size=(n, 10)) * 2 + 1

    def dev(k):
        d = prior(k)
        return {"rand": np.array(d.rand(n, seed=42)), "logpdf": np.array(d.logpdf(x))}

    def orc(k, o):
        d = prior(k)
        return {"rand": o.push_p(d, o.factored_rand(d, n, seed=42)), "logpdf": o.factored_logpdf(d, x)}
    return Case(name, env, dev, orc)


USER_SRC = """
KABC_HD double kabc_user_cost(const double* x, int D, const double* params,
                              const double* data, int64_t ndata, kabc_cost_rng_t* rng) {
    double z0, z1;
    kabc_cost_rng_normal2(rng, &z0, &z1);
    return kabc_fabs(x[0] * x[1] - params[0] + 0.05 * z0) + 0.01 * kabc_fabs(z1);
}"""


def u8_model(k):
    return k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 8), k.costs.Rosenbrock(), 1.0)


def sharded_world1_case(name, N, gens, nt, seed, env):
    def dev(k):
        import torch
        from kissabc_jl_amd.sharded import ShardedAIS
        sh = ShardedAIS(u8_model(k), N, seed=seed, device=torch.device("cuda", 0)).init()
        sh.advance(gens, nt)
        torch.cuda.synchronize()
        return {"x": sh.positions().cpu().numpy(), "stats": _stats(sh.global_stats()), "driver": sh.engine.ens.driver}

    def orc(k, o):
        e = o.OracleAIS(u8_model(k), N, seed=seed).init()
        e.generations_sync(gens, nt, collect=False)
        return {"x": e.state()[0], "stats": _stats(e.stats())}
    return Case(name, env, dev, orc)


def sharded_two_ranks_case(name, N, gens, nt, seed, env):
    """tests/test_gpu_ais_workloads.py test_two_ranks_emulated_on_one_gpu: two world-2 handles on the same halves"""
    def dev(k):
        import torch
        from kissabc_jl_amd.sharded import HipEngine
        dev_ = torch.device("cuda", 0)
        e0 = HipEngine(u8_model(k), N, seed, 0, 2, dev_)
        e1 = HipEngine(u8_model(k), N, seed, 1, 2, dev_, half_buffers=e0.half)
        for e in (e0, e1):
            e.init(100)
            e.synchronize()
        for _ in range(gens):
            for half in (0, 1):
                for e in (e0, e1):
                    e.half_generation(half, nt)
                    e.synchronize()
            for e in (e0, e1):
                e.end_generation(nt)
        x0, lp0, ll0, _ = e0.ens.state()
        x1, lp1, ll1, _ = e1.ens.state()
        q = N // 4
        s0, s1 = e0.stats(), e1.stats()
        return {"x": torch.cat(e0.half, 0).cpu().numpy(), "lp": np.concatenate([lp0[:q], lp1[:q], lp0[q:], lp1[q:]]),
                "ll": np.concatenate([ll0[:q], ll1[:q], ll0[q:], ll1[q:]]),
                "stats": _stats({kk: s0[kk] + s1[kk] for kk in s0}), "driver": e0.ens.driver}

    def orc(k, o):
        e = o.OracleAIS(u8_model(k), N, seed=seed).init()
        e.generations_sync(gens, nt, collect=False)
        x, lp, ll, _ = e.state()
        return {"x": x, "lp": lp, "ll": ll, "stats": _stats(e.stats())}
    return Case(name, env, dev, orc)


# ---- the families ----------------------------------------------------------------------------------------------
def cases(family):
    gauss = lambda k: k.costs.GaussDist([1.0, -0.5])                                       # noqa: E731
    if family == "ais":
        readme = lambda k: k.ApproxKernelizedPosterior(readme_prior(k), k.costs.NormalMeanStdSim(1000, 2.0, 0.04), 0.005)  # noqa: E731
        targets = lambda k: [k.costs.GaussDist([1.0 + 0.3 * c, -0.5 + 0.1 * c]) for c in range(3)]   # noqa: E731
        per_chain = lambda k, c: k.ApproxKernelizedPosterior(n2_prior(k), targets(k)[c], 0.1)        # noqa: E731
        return [
            ais_case("prebuilt_n130", n2_model, 130, 11, 3, 4, {"KABC_AIS_SMALL": "0"}, debug=True, resume=True),
            ais_case("small_readme_n10", readme, 10, 3, 3, 4, {}),
            chains_case("chains3", per_chain, targets, 12, [5, 6, 7], 3, 4, {}),
        ]
    if family == "ais_dyn":
        d20_targets = lambda k: [k.costs.GaussDist(np.full(20, 0.1 * c)) for c in range(5)]          # noqa: E731
        return [
            ais_case("d20_small", d20_model, 60, 21, 3, 2, {}, debug=True),
            ais_case("d20_halves", d20_model, 60, 21, 3, 2, {"KABC_AIS_SMALL": "0"}, debug=True),
            chains_case("d20_chains5", lambda k, c: d20_model(k, 0.1 * c), d20_targets, 60, [11, 12, 13, 14, 15], 3, 2, {}),
            ais_case("d128_many_rounds", d128_model, 140, 21, 2, 2, {"KABC_AIS_SMALL": "1"}),
            ais_case("d34_mixed", d34_model, 100, 21, 3, 2, {}),
        ]
    if family == "smc":
        out = []
        for N in (100, 1000):
            kw = dict(nparticles=N, alpha=0.9, epstol=0.05, seed=5)
            out.append(smc_case(f"loop_{N}", n2_prior, gauss, kw, {"KABC_SMC_LOOP": "1"}))
            out.append(smc_case(f"kernels_{N}", n2_prior, gauss, kw, {"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "0"}))
            out.append(smc_case(f"default_{N}", n2_prior, gauss, kw, {}))
        d20 = lambda k: k.Factored(*[k.Normal(0, 3)] * 20)                                   # noqa: E731
        g20 = lambda k: k.costs.GaussDist(np.full(20, 0.2))                                   # noqa: E731
        out.append(smc_case("dyn_d20", d20, g20, dict(nparticles=500, alpha=0.9, epstol=8.0, seed=5), {}))
        g3 = lambda k: k.costs.GaussDist([0.5, -0.5, 1.0])                                    # noqa: E731
        out.append(smc_case("mvnormal_d3", mv3_prior, g3, dict(nparticles=300, alpha=0.9, epstol=0.2, seed=5), {}))
        out.append(smc_batch_case("batch3", n2_prior, gauss, dict(nparticles=100, alpha=0.9, epstol=0.05), SEEDS3, {}))
        out.append(smc_case("one_exchange_6000", n2_prior, gauss, dict(nparticles=6000, alpha=0.9, epstol=0.05, seed=5),
                            {"KABC_SMC_LOOP": "0", "KABC_SMC_SPEC_SELECT": "1"}))
        d4 = lambda k: k.Factored(*[k.Normal(0, 3)] * 4)                                      # noqa: E731
        g4 = lambda k: k.costs.GaussDist([1.0, -0.5, 0.25, 2.0])                              # noqa: E731
        out.append(recycled_smc_case("recycled_2500", d4, g4, dict(alpha=0.9, epstol=1.0, seed=5), {"KABC_SMC_LOOP": "1"}))
        return out
    if family == "pfilter":
        kw = dict(epstol=0.05, max_iters=12)
        return [
            pf_case("passes0_256", n2_prior, gauss, 256, kw, {"KABC_PF_PASSES": "0"}),
            pf_case("passes1_256", n2_prior, gauss, 256, kw, {"KABC_PF_PASSES": "1"}),
            pf_case("small1_100", n2_prior, gauss, 100, kw, {"KABC_PF_SMALL": "1"}),
            pf_case("small0_100", n2_prior, gauss, 100, kw, {"KABC_PF_SMALL": "0"}),
            pf_case("raised_5", n2_prior, gauss, 5, dict(max_iters=10), {}),
            pf_case("batch3", n2_prior, gauss, 100, kw, {}, seeds=SEEDS3),
        ]
    if family == "abcde":
        g3m2 = lambda k: k.costs.GaussDist([3.0, -2.0])                                       # noqa: E731
        return [
            de_case("small_64", n2_prior, gauss, 0.05, dict(nparticles=64, generations=20), {}),
            de_case("teams_257", n2_prior, gauss, 0.05, dict(nparticles=257, generations=12), {}),
            de_case("blocks_1536", n2_prior, gauss, 0.05, dict(nparticles=1536, generations=8), {}),
            de_case("wavelet_4096_ties", du_prior, g3m2, 0.5, dict(nparticles=4096, generations=6),
                    {"KABC_ABCDE_RANK": "wavelet"}),
            de_case("batch3", n2_prior, gauss, 0.05, dict(nparticles=100, generations=15), {}, seeds=SEEDS3),
        ]
    if family == "reject":
        targets3 = lambda k: [k.costs.GaussDist([1.0 + 0.3 * r, -0.5 + 0.1 * r]) for r in range(3)]   # noqa: E731
        d128 = lambda k: k.Factored(*[k.Normal(0, 1)] * 128)                                  # noqa: E731
        g128 = lambda k: k.costs.GaussDist(np.zeros(128))                                     # noqa: E731
        return [
            reject_case("threshold_fused_d2", n2_prior, gauss, {}, eps=2.0, n=40, draws=3000),
            reject_case("keep_fused_d2", n2_prior, gauss, {}, draws=3000, keep=37),
            reject_case("threshold_phases_d128", d128, g128, {}, eps=11.3, n=40, draws=1000),
            reject_case("keep_phases_d128", d128, g128, {}, draws=1000, keep=37),
            reject_case("overflow_repeat_d2", n2_prior, gauss, {"KABC_REJECT_CAPACITY": "64"}, eps=np.inf, n=1500,
                        draws=1500),
            reject_batch_case("batch_shared_seeds", n2_prior, targets3, [11] * 3, {}, eps=[2.0, 2.5, 3.0], n=40, draws=3000),
            reject_batch_case("batch_shared_seeds_wg", n2_prior, targets3, [11] * 3, {"KABC_REJECT_BATCH_COMPACT": "wg"},
                              draws=3000, keep=37),
            reject_batch_case("batch_distinct_seeds", n2_prior, targets3, SEEDS3, {}, draws=3000, keep=37),
            reject_batch_case("batch_distinct_seeds_wg", n2_prior, targets3, SEEDS3, {"KABC_REJECT_BATCH_COMPACT": "wg"},
                              eps=[2.0, 2.5, 3.0], n=40, draws=3000),
        ]
    if family == "eval_priors":
        banana = lambda k: k.costs.NoisyBanana(0.5)                                           # noqa: E731
        quad = lambda k: k.costs.NoisyQuadDU(5.5)                                             # noqa: E731
        user = lambda k: k.costs.UserCost(USER_SRC, dims=[2], params=[1.5], name="small_prod")   # noqa: E731
        mixed = lambda k: k.Factored(k.Normal(0, 2), k.DiscreteUniform(-3, 3), k.Beta(2.0, 3.0))   # noqa: E731
        g3 = lambda k: k.costs.GaussDist([0.5, 1.0, 0.25])                                    # noqa: E731
        ten = lambda k: k.Factored(k.Uniform(1, 3), k.TruncatedNormal(0, 0.1, 0, 100), k.Beta(15, 2),   # noqa: E731
                                   k.NegativeBinomial(900 / 195, (900 / 195) / (30 + 900 / 195)),
                                   k.DiscreteUniform(1, 10), k.Normal(1, 0.5), k.Gamma(0.4, 3.0),
                                   k.Exponential(2.0), k.LogNormal(0.3, 0.6), k.Beta(0.5, 0.7))
        return [
            evaluate_case("evaluate_63x3", banana, 2, 63, 3, {}),
            evaluate_case("evaluate_200_rows64", quad, 2, 200, 2, {"KABC_EVAL_ROWS": "64"}),
            predictive_case("predictive_mixed", mixed, g3, 100, {}),
            predictive_case("predictive_mixed_rows64", mixed, g3, 200, {"KABC_EVAL_ROWS": "64"}),
            priors_case("factored_rand_logpdf", ten, 300, {}),
            evaluate_case("user_rtc", user, 2, 63, 2, {"KABC_USER_PLUGIN": "hiprtc"}, user=True),
        ]
    if family == "sharded":
        return [
            sharded_world1_case("world1_n256", 256, 3, 4, 5, {}),
            sharded_two_ranks_case("two_ranks_n2048", 2048, 3, 5, 17, {}),
        ]
    raise KeyError(family)


FAMILIES = ("ais", "ais_dyn", "smc", "pfilter", "abcde", "reject", "eval_priors", "sharded")
NEEDS_TORCH = ("sharded",)

# what the cases of a family must report (a case that fell back to another driver is no coverage)
EXPECTED_COURSES = {
    "ais": {"prebuilt_n130.driver": "halves", "prebuilt_n130.driver_resumed": "halves",
            "small_readme_n10.driver": "small", "chains3.driver": "small"},
    "ais_dyn": {"d20_small.driver": "small", "d20_halves.driver": "halves", "d20_chains5.driver": "small",
                "d128_many_rounds.driver": "small", "d34_mixed.driver": "small"},
    "smc": {"loop_100.course": "persistent", "kernels_100.course": "looked", "default_100.course": "persistent",
            "loop_1000.course": "persistent", "kernels_1000.course": "looked", "default_1000.course": "persistent",
            "dyn_d20.course": "looked", "mvnormal_d3.course": "persistent", "batch3.course": "grid",
            "one_exchange_6000.course": "one-exchange", "recycled_2500.course": "persistent"},
    "pfilter": {"batch3.course": "grid"},
    "abcde": {"batch3.course": "grid"},
    "reject": {"threshold_fused_d2.course": "fused", "keep_fused_d2.course": "fused",
               "threshold_phases_d128.course": "phases", "keep_phases_d128.course": "phases",
               "overflow_repeat_d2.course": "fused",
               "batch_shared_seeds.course": "table", "batch_shared_seeds_wg.course": "table",
               "batch_distinct_seeds.course": "grid", "batch_distinct_seeds_wg.course": "grid"},
    "eval_priors": {},
    "sharded": {"world1_n256.driver": "halves", "two_ranks_n2048.driver": "halves"},
}
# launch counts the cases must show (the path was taken, not skipped by the poisoned and the plain run alike):
# the overflow-repeat call needs the launch that overflowed and its pieces; 200 rows in launches of 64 are 4
EXPECTED_MIN_LAUNCHES = {"reject": {"overflow_repeat_d2.launches": 2}, "eval_priors": {"predictive_mixed_rows64.launches": 4}}


class DeviceFault(RuntimeError):
    """a case ended with a device / HIP error: `partial` holds what ran before it; nothing more may start"""

    def __init__(self, text, partial):
        super().__init__(text)
        self.partial = partial


def _is_device_error(k, e):
    from kissabc_jl_amd import _cdefs as cd
    text = str(e)
    return (isinstance(e, k.KabcError) and getattr(e, "status", None) == cd.KABC_ERR_DEVICE) or "HIP error" in text \
        or "hipError" in text or "illegal memory access" in text


def run_family(k, family):
    """every case of the family on the device: {"<case>.<key>": array}; a case that raises leaves "<case>.error".
    A device / HIP error ends the family there (DeviceFault): no further case runs on a card that has faulted."""
    out = {}
    for c in cases(family):
        with knobs(c.env):
            try:
                for key, v in c.dev(k).items():
                    out[f"{c.name}.{key}"] = np.asarray(v)
            except Exception as e:                       # (the parent fails on it)
                out[f"{c.name}.error"] = np.asarray(f"{type(e).__name__}: {e}")
                if _is_device_error(k, e):
                    raise DeviceFault(f"{family}.{c.name}: {type(e).__name__}: {e}", out)
    return out


def run_probe(k):
    ctx = k.Context(0)
    fresh, pooled, recycled, (byte, was_recycled) = k._lib.poison_probe(PROBE_BYTES, ctx)
    ctx.close()
    return {"probe.fresh": fresh, "probe.pooled": pooled, "probe.recycled": recycled,
            "probe.info": np.array([byte, was_recycled], dtype=np.int64)}


def main(argv):
    family, path = argv[1], argv[2]
    sys.path.insert(0, ROOT)
    import kissabc_jl_amd as k
    status = 0
    try:
        out = run_probe(k)
        out.update(run_family(k, family))
    except DeviceFault as e:
        out, status = e.partial, DEVICE_FAULT_STATUS
        sys.stderr.write(f"device error, nothing more is run: {e}\n")
    with open(path, "wb") as f:
        np.savez(f, **out)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
