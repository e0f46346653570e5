"""Loader of the C-ABI library (kissabc.jl_amd/lib/libkabc_hip.so).

There is NO fallback: if the HIP extension is missing or no gfx950 device is
visible, the product path raises.  (The CPU oracle lives under oracle/ and is
only ever used by tests/, smoke() and bench.py's cpu_baseline leg.)
"""
import ctypes as C
import contextlib
import os
import signal
import threading

from . import _cdefs

_HERE = os.path.dirname(os.path.abspath(__file__))
# KABC_PROBES=1 selects the build with the timing probes of tools/ compiled into the AIS
# kernel (make -C kissabc.jl_amd/csrc PROBES=1; built on first use)
PROBES = os.environ.get("KABC_PROBES") == "1"
LIB_PATH = os.path.join(_HERE, "lib", "libkabc_hip_probes.so" if PROBES else "libkabc_hip.so")
# KABC_LIB: an experimental build of the library (make VARIANT=...), for A/B runs on one box
LIB_PATH = os.environ.get("KABC_LIB") or LIB_PATH
_lib = None


class KabcError(RuntimeError):
    """Raised for every non-zero kabc_status_t; .status holds the code and the
    message is the library's (for reference-defined errors: the reference's text)."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


class Cancelled(KabcError):
    """KABC_ERR_CANCELLED: the call stopped at a generation / iteration boundary because
    Context.cancel() was called (include/kabc.h: what the handle or result then holds)."""


def _preload_torch_hip():
    # KABC_NO_TORCH_PRELOAD=1: hosts that never import torch (bench.py, the RCCL tests) keep
    # the process on the system ROCm runtime alone
    if os.environ.get("KABC_NO_TORCH_PRELOAD") == "1":
        return
    _preload_torch_hip_impl()


def _preload_torch_hip_impl():
    """PyTorch wheels bundle their own ROCm runtime (libamdhip64 & co).  If this
    library pulls in the system libamdhip64 first, a later `import torch` binds to a
    mixed set of ROCm libraries and reports "No HIP GPUs are available".  Loading
    torch first makes both use torch's copy (same soname).  Only done when torch is
    installed; the C ABI itself never needs torch."""
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass


def load():
    global _lib
    if _lib is None:
        _preload_torch_hip()
        if PROBES and not os.path.exists(LIB_PATH):
            import subprocess
            subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "PROBES=1",
                            f"-j{min(32, os.cpu_count() or 8)}"], check=True)
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C kissabc.jl_amd/csrc`). The KissABC MI355X path has no "
                "CPU fallback.")
        _lib = _cdefs.bind(C.CDLL(LIB_PATH))
    return _lib


def check(status):
    if status != 0:
        msg = load().kabc_last_error()
        cls = Cancelled if status == _cdefs.KABC_ERR_CANCELLED else KabcError
        raise cls(status, msg.decode("utf-8", "replace") if msg else f"kabc status {status}")


class Context:
    """kabc_ctx_t: one GPU + one HIP stream."""

    def __init__(self, device=0, stream=None, _borrowed=None):
        lib = load()
        self._owned = _borrowed is None
        if _borrowed is not None:   # a context owned by a communicator (kabc_comm_init_all)
            self._h = C.c_void_p(_borrowed)
        else:
            self._h = C.c_void_p()
            check(lib.kabc_ctx_create(int(device), C.c_void_p(stream) if stream else None,
                                      C.byref(self._h)))
        self.device = device

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        check(load().kabc_ctx_synchronize(self._h))

    def cancel(self):
        """Request that the call running on this context stop at its next generation / iteration
        boundary; it then raises Cancelled.  Safe from any thread (e.g. a threading.Timer).  The
        request is sticky: made while the context is idle, it cancels the next call."""
        check(load().kabc_ctx_cancel(self._h))

    def clear_cancel(self):
        """Drop a pending cancel request."""
        check(load().kabc_ctx_clear_cancel(self._h))

    @contextlib.contextmanager
    def interruptible(self):
        """Around a blocking library call: Ctrl-C cancels the call (it stops at its next boundary)
        and then raises KeyboardInterrupt as usual.  Arming is one sigaction look and a store."""
        lib = load()
        arm = threading.current_thread() is threading.main_thread()
        if arm:
            check(lib.kabc_ctx_cancel_on_sigint(self._h, 1))
        try:
            yield
        finally:
            if arm and lib.kabc_ctx_cancel_on_sigint(self._h, 0) == _cdefs.KABC_ERR_CANCELLED:
                # the signal was held back from Python's handler while the call ran: deliver it now
                # (KeyboardInterrupt, or whatever handler the program installed); it replaces the
                # Cancelled the call raised
                signal.raise_signal(signal.SIGINT)

    def close(self):
        if self._h and self._owned:
            release_pinned_cache()   # (page-locked result blocks kept for reuse go with the context)
            load().kabc_ctx_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


# Page-locked blocks whose arrays have died, kept for the next result of the same size: pinning
# 268 MB (an smc result at 2 M particles x 16) costs as much as copying into it ten times.
_pinned_free = {}            # nbytes -> [address, ...]
_pinned_free_bytes = 0
_pinned_lock = threading.RLock()   # (re-entrant: a GC pass inside the locked region may finalise another block)


def _pinned_cache_cap():
    """KABC_PINNED_CACHE_MB (default 1024): page-locked bytes kept on the free list"""
    return int(float(os.environ.get("KABC_PINNED_CACHE_MB", "1024")) * (1 << 20))


def release_pinned_cache():
    """Hand every cached page-locked block back to the driver (also done when a Context closes)."""
    global _pinned_free_bytes
    with _pinned_lock:
        blocks = [p for lst in _pinned_free.values() for p in lst]
        _pinned_free.clear()
        _pinned_free_bytes = 0
    if _lib is not None:
        for p in blocks:
            _lib.kabc_host_free(C.c_void_p(p))


class _PinnedBlock:
    """One kabc_host_alloc allocation; when the last numpy view dies it goes back to the free list
    (or to the driver, beyond KABC_PINNED_CACHE_MB)."""

    def __init__(self, nbytes):
        global _pinned_free_bytes
        with _pinned_lock:
            lst = _pinned_free.get(nbytes)
            if lst:
                self.ptr, self.nbytes = lst.pop(), nbytes
                _pinned_free_bytes -= nbytes
                return
        p = C.c_void_p()
        check(load().kabc_host_alloc(C.c_size_t(nbytes), C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def __del__(self):
        global _pinned_free_bytes
        try:
            if self.ptr and _lib is not None:
                with _pinned_lock:
                    keep = _pinned_free_bytes + self.nbytes <= _pinned_cache_cap()
                    if keep:
                        _pinned_free.setdefault(self.nbytes, []).append(self.ptr)
                        _pinned_free_bytes += self.nbytes
                if not keep:
                    _lib.kabc_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass
        self.ptr = None


def pinned_empty(shape, dtype="float64"):
    """numpy array over page-locked host memory (kabc_host_alloc): the destination of
    the sample trace, so that kabc_ais_advance can DMA it while the kernels run, and of large
    smc / ABCDE results.  Falls back to ordinary memory when pinning fails or KABC_PINNED_TRACE=0."""
    import numpy as np
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    if n == 0 or os.environ.get("KABC_PINNED_TRACE", "1") == "0":
        return np.empty(shape, dtype=dt)
    try:
        blk = _PinnedBlock(n)
    except KabcError:
        return np.empty(shape, dtype=dt)
    buf = (C.c_char * n).from_address(blk.ptr)
    buf._kabc_block = blk
    return np.frombuffer(buf, dtype=dt).reshape(shape)


def result_empty(shape, dtype="float64"):
    """destination of a result copy: page-locked from 1 MiB on (the copy then runs at the PCIe
    rate instead of faulting fresh pages in one by one), ordinary memory below"""
    import numpy as np
    dt = np.dtype(dtype)
    if int(np.prod(shape)) * dt.itemsize >= (1 << 20):
        return pinned_empty(shape, dt)
    return np.empty(shape, dtype=dt)


MATH_FN = {"log": 0, "exp": 1, "log1p": 2, "lgamma": 3, "sincos2pi": 4, "sqrt": 5, "rint": 6,
           "log_pn": 7, "sqrt_pn": 8, "u01": 9, "normal_pair": 10, "index32": 11,
           "exp_bounded": 12}


def math_probe(name, x, ctx=None):
    """kabc_math_probe: one include/kabc_math.h function evaluated on the device
    (verification only; 64-bit words travel as the bit patterns of doubles)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size // (2 if name in ("normal_pair", "index32") else 1)
    ow = 2 if name in ("sincos2pi", "normal_pair") else 1
    out = np.empty(n * ow)
    ctx = ctx or default_context()
    check(load().kabc_math_probe(ctx.handle, MATH_FN[name], n,
                                 x.ctypes.data_as(_cdefs.c_double_p),
                                 out.ctypes.data_as(_cdefs.c_double_p)))
    return out.reshape(-1, 2) if ow == 2 else out


# the tables of prebuilt kernels (include/kabc.h KABC_PREBUILT_*)
PREBUILT_FAMILY = {"AIS_HALF": 1, "AIS_WIDE": 2, "AIS_SMALL": 3, "SMC_PHASES": 4, "SMC_LOOP": 5, "SMC_SMALL": 6,
                   "ABCDE_GEN": 7, "ABCDE_SMALL": 8, "PF_PHASES": 9, "PF_SMALL": 10, "PF_BATCH": 11}


def prebuilt_has(family, cost_id, D, variant):
    """kabc_prebuilt_has (verification only; no device): does the table `family` hold a kernel for
    (cost id, D, variant)?  variant: AIS, pcx = prior class + 4 * (posterior kind - 1); smc, 1 simple, 0 general;
    ABCDE and pfilter, 0."""
    return bool(load().kabc_prebuilt_has(PREBUILT_FAMILY.get(family, family), int(cost_id), int(D), int(variant)))


def last_kernel(ctx=None):
    """kabc_ctx_last_kernel (verification only): (family, cost id, D, prior class or simple flag, posterior
    kind, waves per workgroup) of the last prebuilt AIS / smc launch on the context; zeros for any other kernel.
    ABCDE and pfilter: (family, cost id, D, sub-course, 0, waves per workgroup), include/kabc.h."""
    info = (C.c_int32 * 6)()
    ctx = ctx or default_context()
    load().kabc_ctx_last_kernel(ctx.handle, info)
    return tuple(int(v) for v in info)


_poison_byte = ()            # (KABC_POISON_ALLOC as it stood at the first question: once per process, as in the library)


def poison_byte_requested():
    """The byte the library's working buffers are filled with (KABC_POISON_ALLOC), None when the hook is
    off.  Read once per process, like the library's own look at the variable."""
    global _poison_byte
    if _poison_byte == ():
        _poison_byte = poison_byte_rule(os.environ.get("KABC_POISON_ALLOC"))
    return _poison_byte


def poison_byte_rule(e):
    """The library's rule (csrc/host_common.hpp poison_byte): None when off (unset, empty, a leading 0
    that is no 0xNN), 0xNN that byte, anything else 0xA5."""
    if not e:
        return None
    if e[:2] in ("0x", "0X"):
        digits = e[2:]
        ok = 1 <= len(digits) and all(ch in "0123456789abcdefABCDEF" for ch in digits)
        return int(digits, 16) if ok and int(digits, 16) <= 0xFF else 0xA5
    return None if e[0] == "0" else 0xA5


def poison_probe(n, ctx=None):
    """kabc_poison_probe (verification only): the bytes of a fresh working buffer, of a first
    buffer from the context's pool and of the recycled one a second allocation got, as uint8
    arrays of n, plus (byte in force or -1, whether the second allocation was recycled)."""
    import numpy as np
    n = int(n)
    fresh, pooled, recycled = (np.empty(max(n, 0), dtype=np.uint8) for _ in range(3))
    info = (C.c_int32 * 2)()
    ctx = ctx or default_context()
    u8 = C.POINTER(C.c_uint8)
    check(load().kabc_poison_probe(ctx.handle, n, fresh.ctypes.data_as(u8), pooled.ctypes.data_as(u8),
                                   recycled.ctypes.data_as(u8), info))
    return fresh, pooled, recycled, (int(info[0]), int(info[1]))
