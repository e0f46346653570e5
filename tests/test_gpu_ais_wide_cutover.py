"""-m gpu: from how many sub-steps the default rule (no KABC_AIS_WIDE) takes the wide AIS
half-generation kernel, by prior class (csrc/capi_ais.hip ais_use_wide): 12 for the classes whose wide
kernels have the short first chunk and the cut prologue (BOX here), 24 for the SIMPLE class, whose wide
kernels keep the prologue that was measured to lose below 24.  Which kernel ran is read from
kabc_ctx_last_kernel.  The launch is the smallest the rule accepts on a 256-unit device (the
MI355X's): two batches per compute unit and half, as in test_gpu_ais_wide.py's default-dispatch case.
Same bits either way: the forced geometries are compared elsewhere (test_gpu_ais_wide3.py)."""
import pytest

pytestmark = pytest.mark.gpu

N = 2 * 2 * 64 * 256


def _models(k):
    return {
        "box8": k.ApproxKernelizedPosterior(k.Factored(*[k.Uniform(-5, 5)] * 8), k.costs.Rosenbrock(), 1.0),
        "simple4": k.ApproxKernelizedPosterior(
            k.Factored(k.Uniform(-3, 3), k.Normal(0, 2), k.TruncatedNormal(0, 2, -3, 3), k.Uniform(-4, 4)),
            k.costs.Rosenbrock(), 1.0),
    }


@pytest.mark.parametrize("name,nt,wide", [("box8", 11, False), ("box8", 12, True), ("box8", 16, True),
                                          ("simple4", 12, False), ("simple4", 23, False), ("simple4", 24, True)])
def test_default_rule_by_prior_class(k, gpu_ctx, monkeypatch, name, nt, wide):
    from kissabc_jl_amd import _lib
    monkeypatch.setenv("KABC_AIS_SMALL", "0")
    monkeypatch.setenv("KABC_SPECIALIZE", "0")
    monkeypatch.delenv("KABC_AIS_WIDE", raising=False)
    ens = k.AisEnsemble(_models(k)[name], N, seed=3).init()
    assert ens.driver == "halves"
    ens.advance(1, nt)
    got = _lib.last_kernel(ens.ctx)
    ens.close()
    family = _lib.PREBUILT_FAMILY["AIS_WIDE" if wide else "AIS_HALF"]
    assert got[0] == family and got[2] == (8 if name == "box8" else 4), (name, nt, got)
    assert got[3] == (0 if name == "box8" else 1), (name, nt, got)   # prior class: BOX 0, SIMPLE 1
    assert got[5] == (12 if wide else 4), (name, nt, got)
