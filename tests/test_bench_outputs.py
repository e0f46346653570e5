"""bench.py --steps / --dump-outputs: the timed steps are exactly --steps, and the outputs of the timed
path are written as float64 .npy files within a byte budget.  CPU: the writer on a stand-in ensemble.
GPU: two runs with the same arguments dump the same bits, and so do a plain and a --full run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _StandIn:
    def __init__(self, n, d):
        self.n, self.d = n, d

    def state(self):
        r = np.random.default_rng(3)
        return r.normal(size=(self.n, self.d)), r.normal(size=self.n), r.normal(size=self.n), 0


def _bench_module(monkeypatch):
    monkeypatch.setenv("KABC_NO_TORCH_PRELOAD", os.environ.get("KABC_NO_TORCH_PRELOAD", "1"))
    import bench
    return bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_state_as_float64(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    ens = _StandIn(4096, 8)
    bench.dump_outputs(str(tmp_path), ens, {"proposals": 10, "cost_evals": 9, "accepted": 3}, 0, 1, False)
    got = _load(tmp_path)
    assert set(got) == {"walkers", "logprior", "loglik", "counters"}
    assert all(a.dtype == np.float64 for a in got.values())
    x, lp, ll, _ = ens.state()
    assert np.array_equal(got["walkers"], x) and np.array_equal(got["logprior"], lp)
    assert np.array_equal(got["loglik"], ll) and got["counters"].tolist() == [10, 9, 3]


def test_dump_outputs_samples_fixed_rows_beyond_the_budget(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    ens = _StandIn(65536, 8)   # 5 MiB of state
    st = {"proposals": 1, "cost_evals": 1, "accepted": 0}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ens, st, 0, 1, False)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 1 << 20
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["rows"].astype(np.int64)
    assert np.array_equal(a["rows"], b["rows"]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["walkers"], ens.state()[0][rows])
    # a sharded rank writes its own rows under its own names, within its share of the budget
    bench.dump_outputs(str(tmp_path / "s"), ens, st, 3, 4, True)
    assert sorted(os.listdir(tmp_path / "s")) == ["loglik_rank3.npy", "logprior_rank3.npy", "rows_rank3.npy",
                                                  "walkers_rank3.npy"]
    assert sum(f.stat().st_size for f in (tmp_path / "s").iterdir()) <= (1 << 20) // 4


@pytest.mark.gpu
def test_bench_times_exactly_steps_and_dumps_the_same_outputs_twice(tmp_path, gpu_ctx):
    steps, warmup = 7, 2
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", str(warmup), "--no-alt", "--no-smc", "--no-cpu-baseline",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    for line in lines:
        h = line["by_ntransitions"]["100"]
        assert line["steps"] == steps and h["steps"] * h["blocks"] == steps
        assert line["ms_per_step"] > 0 and abs(line["ms_per_step"] - h["timed_s"] * 1e3 / steps) < 1e-9
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"walkers", "logprior", "loglik", "counters"}
    assert a["walkers"].shape == (65536, 8) and np.all(np.isfinite(a["walkers"]))
    assert a["counters"][0] == 65536 * 100 * (warmup + steps)
    for name in a:
        assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), name


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_from_the_state_a_full_run_times(tmp_path, gpu_ctx):
    """A plain run reports the headline only; --full adds the other settings and legs.  Both time the
    headline on the same ensemble (a plain run takes the other settings' steps untimed), so they dump
    the same bits."""
    steps, warmup = 7, 2
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-smc", "--no-cold-spec"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", str(warmup), "--dump-outputs", str(tmp_path / name), *extra],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert set(plain["by_ntransitions"]) == {"100"} and set(full["by_ntransitions"]) == {"1", "16", "100"}
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert not {"cpu_baseline", "smc_c4", "readme_c1", "c2", "by_prior_class", "value_survey_8d"} & set(plain)
    assert {"readme_c1", "c2", "by_prior_class", "value_survey_8d"} <= set(full)
    for line in (plain, full):
        assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["roofline"]["frac"] > 0
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert a["counters"][0] == 65536 * ((1 + 16) * (5 + steps) + 100 * (warmup + steps))
    for name in a:
        assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), name
