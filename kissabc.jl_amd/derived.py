"""Derived: a user-defined map g(θ) from a trace row to G derived values, evaluated on the device -- what the
reference's caller writes as `P[1] / P[2]`, `P[1] > P[2]` or `sqrt(P[1]^2 + P[2]^2)` on the Particles that
sample() returns.  A C snippet (include/kabc.h, "user-defined derived quantities"), compiled in process by
hipRTC like a cost snippet; applied to rows on the host's request (d(theta), kabc_derived_eval) or to every
row of a summarised trace on the device (summary_begin(derived=d), sample(..., summary=True, derived=d))."""
import ctypes as C

import numpy as np

from . import _cdefs as cd

_registered = {}


def _range_side(v, G, name):
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"Derived: hist_range: {name} must be a scalar or [G] = [{G}] of numbers, not {v!r}") from None
    if a.shape not in ((), (G,)):
        raise ValueError(f"Derived: hist_range: {name} must be a scalar or [G] = [{G}], not of shape {list(a.shape)}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"Derived: hist_range: {name} must be finite")
    return np.ascontiguousarray(np.broadcast_to(a, (G,)))


class Derived:
    """`source` must define

        KABC_HD void kabc_user_derived(const double* x, int D, const double* params, int nparams,
                                       double* g, int G)

    writing all G entries of g from the row x (kabc_math.h is available: kabc_sqrt, kabc_log, kabc_exp, ...; no
    random stream).  `G`: 1 ... KABC_MAX_DIM_DYN.  `params`: the doubles the snippet reads.  `names`: G labels
    for the summary (default g0, g1, ...).  `hist_range`: (lo, hi) of scalars or [G], the range of the derived
    histograms; None takes the automatic convention applied to d(walkers) when the summary is opened.

    The snippet is checked at once (kabc_compile_derived): a syntax error or a missing kabc_user_derived raises
    KabcError with the compiler's message."""

    def __init__(self, source, G, params=(), names=None, hist_range=None):
        if not isinstance(source, str) or not source.strip():
            raise ValueError("Derived: source must be the C text of kabc_user_derived")
        if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or not 1 <= int(G) <= cd.KABC_MAX_DIM_DYN:
            raise ValueError(f"Derived: G must be an int in 1 ... {cd.KABC_MAX_DIM_DYN}, not {G!r}")
        self.G = int(G)
        try:
            p = np.asarray(params, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"Derived: params must be a sequence of numbers, not {params!r}") from None
        if p.ndim > 1:
            raise ValueError(f"Derived: params must be a flat sequence, not of shape {list(p.shape)}")
        self.params = np.ascontiguousarray(p.ravel())
        if names is None:
            names = [f"g{j}" for j in range(self.G)]
        names = list(names)
        if len(names) != self.G or not all(isinstance(s, str) for s in names):
            raise ValueError(f"Derived: names must be {self.G} strings, not {names!r}")
        self.names = tuple(names)
        if hist_range is not None:
            if not isinstance(hist_range, (tuple, list)) or len(hist_range) != 2:
                raise ValueError(f"Derived: hist_range must be None or (lo, hi), not {hist_range!r}")
            lo, hi = _range_side(hist_range[0], self.G, "lo"), _range_side(hist_range[1], self.G, "hi")
            if not np.all(lo < hi):
                j = int(np.argwhere(~(lo < hi))[0][0])
                raise ValueError(f"Derived: hist_range: derived value {j}: lo = {float(lo[j])!r} is not below "
                                 f"hi = {float(hi[j])!r}")
            hist_range = (lo, hi)
        self.hist_range = hist_range
        self.source = source
        from . import _lib
        did = _registered.get(source)
        if did is None:
            out = C.c_int32()
            _lib.check(_lib.load().kabc_compile_derived(source.encode(), C.byref(out)))
            did = _registered[source] = out.value
        self.id = did

    def _params_ptr(self):
        return self.params.ctypes.data_as(cd.c_double_p) if self.params.size else None

    def evaluate(self, theta, ctx=None):
        """g at given rows, on the GPU (kabc_derived_eval): `theta` is one row [D] or rows [n][D] -- a returned
        trace, smc(...).info["theta_all"], anything; leading axes beyond two are kept ([...][D] -> [...][G]).
        The same bits the device summary folds for those rows."""
        from . import _lib
        a = np.asarray(theta, dtype=np.float64)
        if a.ndim < 1 or a.shape[-1] < 1:
            raise ValueError("theta is one row [D] or rows [...][D], D >= 1")
        D = a.shape[-1]
        if D > cd.KABC_MAX_DIM_DYN:
            raise ValueError(f"length(θ) = {D} outside 1..{cd.KABC_MAX_DIM_DYN}")
        rows = np.ascontiguousarray(a.reshape(-1, D))
        n = rows.shape[0]
        out = _lib.result_empty((n, self.G))
        ctx = ctx or _lib.default_context()
        with ctx.interruptible():
            _lib.check(_lib.load().kabc_derived_eval(ctx.handle, self.id, D, self.G, n,
                                                     rows.ctypes.data_as(cd.c_double_p), self._params_ptr(),
                                                     self.params.size, out.ctypes.data_as(cd.c_double_p)))
        return out.reshape(a.shape[:-1] + (self.G,))

    __call__ = evaluate

    def __repr__(self):
        return f"Derived({', '.join(self.names)})"
