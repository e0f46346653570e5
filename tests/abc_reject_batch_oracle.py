"""abc_reject_batch restated on the CPU oracle (helper of tests/test_abc_reject_batch_args.py and
tests/test_gpu_abc_reject_batch.py).  Run r of a batch is abc_reject with costs[r], seeds[r], eps[r]; its result is
a selection (select_threshold / select_keep of tests/abc_reject_oracle.py) of the rows of its own oracle table.  Runs
that share a seed share the table's theta and log-prior columns -- checked here, not assumed."""
import numpy as np

from abc_reject_oracle import oracle_table, select_keep, select_threshold


def batch_tables(orc, prior, costs, draws, seeds, first_row=0):
    """[(P, logprior, C)] per run, each from its own oracle calls"""
    return [oracle_table(orc, prior, c, draws, s, first_row) for c, s in zip(costs, seeds)]


def expected_batch(tables, eps=None, n=None, keep=None):
    """per run: dict(P, C, logprior, eps, index, draws, exhausted) as abc_reject returns them"""
    out = []
    for r, (P, lp, C) in enumerate(tables):
        if keep is not None:
            idx, e = select_keep(C, keep)
            d, ex = len(C), False
        else:
            e = float(eps[r] if np.ndim(eps) else eps)
            idx, d, ex = select_threshold(C, e, n)
        out.append(dict(P=P[idx], C=C[idx], logprior=lp[idx], eps=e, index=idx, draws=d, exhausted=ex))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_run_equals(got, want, what=""):
    """a RejectResult (return_array=True) against an expected_batch entry or another RejectResult, on bit patterns"""
    if not isinstance(want, dict):
        want = dict(P=want.P, C=want.C, logprior=want.logprior, eps=want.eps, index=want.info["index"],
                    draws=want.info["draws"], exhausted=want.info["exhausted"])
    assert np.array_equal(got.info["index"], want["index"]), (what, got.info["index"][:8], want["index"][:8])
    D = np.asarray(got.P).shape[-1] if np.asarray(got.P).ndim == 2 else 1
    assert same_bits(np.asarray(got.P).reshape(-1, D), np.asarray(want["P"]).reshape(-1, D)), what
    assert same_bits(got.C, want["C"]), what
    assert same_bits(got.logprior, want["logprior"]), what
    assert same_bits([got.eps], [want["eps"]]), (what, got.eps, want["eps"])
    assert got.info["draws"] == want["draws"], (what, got.info["draws"], want["draws"])
    assert got.info["exhausted"] == want["exhausted"], what
