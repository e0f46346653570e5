"""-m gpu: every device driver on poisoned working memory.

Fresh device memory nearly always reads as zero, so a kernel that forgets to initialise a counter, a flag, an
accumulator or a padding row passes every other test.  KABC_POISON_ALLOC (csrc/host_common.hpp) fills every
working buffer -- fresh, or recycled from a context's pool -- with one byte before use; it is read once per
process, so each family of cases (tests/poison_child.py) runs in a child process of its own, under byte 0xA5
(all integers large and odd-looking, doubles about -2^-421) and under 0xFF (NaN doubles, all-ones integers).

For every case the child's arrays and scalars must equal the CPU oracle's bit for bit (uint64 views: NaN and
Inf included) and the same call made unpoisoned in this process.  The probe bytes (kabc_poison_probe) must show
the requested byte in a fresh and in a recycled buffer -- a typo in the variable's name would otherwise make
every test here pass vacuously -- and the drivers and courses the cases report must be the expected ones: a
case that fell back to another driver is no coverage.  One more child runs the smc family under 0xA5 with
KABC_POOL_MB=0 (read once per process too): nothing is pooled, the results -- the larger-then-smaller sequence
on one context among them -- are the same.

One child runs at a time under its own time limit; after a child that ends abnormally (time limit, signal,
abort, or the child's own status for a device / HIP error in one of its cases) nothing more is started on the
GPU -- neither a child nor a run of this process -- and the remaining families fail as "not run".  Nothing is
retried."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import poison_child as pc

pytestmark = pytest.mark.gpu

PATTERNS = {"a5": ("1", 0xA5), "ff": ("0xff", 0xFF), "a5_pool_off": ("1", 0xA5)}
POOL_OFF = ("a5_pool_off", "smc")      # this child runs with KABC_POOL_MB=0
RUNS = [(pat, fam) for pat in ("a5", "ff") for fam in pc.FAMILIES] + [POOL_OFF]
CHILD_TIMEOUT_S = 300
ABNORMAL = (134, 137, 139, pc.DEVICE_FAULT_STATUS)
_STOPPED = []                 # why nothing more may start on the GPU (a child or a run of this process faulted)


@contextlib.contextmanager
def _no_specialisation():
    """the prebuilt kernels are what is tested: no run-time specialised unit takes over half way"""
    old = os.environ.get("KABC_SPECIALIZE")
    os.environ["KABC_SPECIALIZE"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("KABC_SPECIALIZE", None)
        else:
            os.environ["KABC_SPECIALIZE"] = old


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{(pattern, family): ("ok", arrays) | ("failed", text)}: the children in order, stopping at the first
    abnormal end"""
    tmp = tmp_path_factory.mktemp("poison")
    out = {}
    for pat, fam in RUNS:
        if _STOPPED:
            out[pat, fam] = ("failed", f"not run after {_STOPPED[0]}")
            continue
        path = str(tmp / f"{pat}_{fam}.npz")
        env = {a: b for a, b in os.environ.items() if a not in pc.KNOBS and a != "KABC_POOL_MB"}
        env.update(KABC_POISON_ALLOC=PATTERNS[pat][0], KABC_SPECIALIZE="0")
        if fam not in pc.NEEDS_TORCH:
            env["KABC_NO_TORCH_PRELOAD"] = "1"
        if (pat, fam) == POOL_OFF:
            env["KABC_POOL_MB"] = "0"
        cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(pc.__file__)), "poison_child.py"), fam, path]
        try:
            r = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT_S, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _STOPPED.append(f"{fam} ({pat}) ended with a timeout of {CHILD_TIMEOUT_S} s")
            out[pat, fam] = ("failed", _STOPPED[0])
            continue
        if r.returncode < 0 or r.returncode in ABNORMAL:
            _STOPPED.append(f"{fam} ({pat}) ended with status {r.returncode}")
            out[pat, fam] = ("failed", _STOPPED[0] + "\n" + r.stderr[-2000:])
        elif r.returncode != 0:
            out[pat, fam] = ("failed", f"status {r.returncode}\n{r.stderr[-2000:]}")
        else:
            with np.load(path) as z:
                out[pat, fam] = ("ok", {key: z[key] for key in z.files})
    return out


@pytest.fixture(scope="module")
def expected(k, orc, gpu_ctx):
    """per family, computed once: the oracle's arrays and the unpoisoned device run of this process"""
    cache = {}

    def get(fam):
        if fam not in cache:
            ref = {}
            for c in pc.cases(fam):
                for key, v in c.orc(k, orc).items():
                    ref[f"{c.name}.{key}"] = np.asarray(v)
            assert not _STOPPED, f"not run after {_STOPPED[0]}"
            with _no_specialisation():
                try:
                    cache[fam] = (ref, pc.run_family(k, fam))
                except pc.DeviceFault as e:
                    _STOPPED.append(f"the unpoisoned run of this process ended with a device error: {e}")
                    raise
        return cache[fam]
    return get


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _report_keys(arrays):
    return {key for key in arrays if key.rsplit(".", 1)[1].startswith(("driver", "course"))}


def _child(children, pat, fam):
    kind, got = children[pat, fam]
    assert kind == "ok", got
    return got


@pytest.mark.parametrize("pat,fam", RUNS)
def test_poisoned_run_equals_oracle(children, expected, pat, fam):
    got = _child(children, pat, fam)
    ref, plain = expected(fam)
    errors = {key: str(v) for key, v in list(got.items()) + list(plain.items()) if key.endswith(".error")}
    assert not errors, errors
    assert ref, fam
    for key, want in ref.items():
        assert key in got and key in plain, key
        assert _same_bits(plain[key], want), f"unpoisoned {key} differs from the oracle"
        assert _same_bits(got[key], want), f"poisoned ({pat}) {key} differs from the oracle"
    # what the oracle does not give (launch counts, reported drivers): equal to the unpoisoned run
    for key in plain:
        if key not in ref:
            assert key in got and np.array_equal(got[key], plain[key]), key
    # ... and the launch counts show the path was taken (not skipped by both runs alike)
    for key, least in pc.EXPECTED_MIN_LAUNCHES.get(fam, {}).items():
        assert int(got[key]) >= least and int(plain[key]) >= least, (key, got[key], plain[key])


@pytest.mark.parametrize("pat,fam", RUNS)
def test_poison_was_in_force(children, pat, fam):
    got = _child(children, pat, fam)
    byte = PATTERNS[pat][1]
    n = pc.PROBE_BYTES
    want = np.full(n, byte, dtype=np.uint8)
    assert int(got["probe.info"][0]) == byte
    assert np.array_equal(got["probe.fresh"], want)
    assert np.array_equal(got["probe.pooled"], want)
    if (pat, fam) == POOL_OFF:      # nothing is pooled: the second allocation is a fresh one of n - n / 4 bytes
        assert int(got["probe.info"][1]) == 0
        want[n - n // 4:] = 0
    else:                           # the first owner's buffer, which it left full of 0x3C, poisoned over its whole size
        assert int(got["probe.info"][1]) == 1
    assert np.array_equal(got["probe.recycled"], want)


def test_probe_unpoisoned(k, gpu_ctx):
    """this process runs without the variable: the hook is off, and the recycled buffer shows the bytes its
    first owner left (so the poisoned children's recycled bytes do come from the hook)"""
    assert "KABC_POISON_ALLOC" not in os.environ
    ctx = k.Context(0)
    fresh, pooled, recycled, (byte, was_recycled) = k._lib.poison_probe(pc.PROBE_BYTES, ctx)
    ctx.close()
    assert byte == -1 and was_recycled == 1
    assert np.array_equal(recycled, np.full(pc.PROBE_BYTES, 0x3C, dtype=np.uint8))


@pytest.mark.parametrize("pat", ["a5", "ff", "a5_pool_off"])
def test_drivers_and_courses_are_the_expected_set(children, pat):
    seen = {}
    fams = [f for p_, f in RUNS if p_ == pat]
    for fam in fams:
        got = _child(children, pat, fam)
        seen[fam] = {key: str(got[key]) for key in sorted(_report_keys(got))}
    assert seen == {fam: pc.EXPECTED_COURSES[fam] for fam in fams}
