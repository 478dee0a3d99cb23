"""bench.py's plain run and --dump-outputs: what a plain run leaves out (the --full legs), that --steps
sets the number of timed steps, and that the dumped arrays are what the timed path hands its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Under the byte budget every row is written; over it, a sorted row sample that is the same on every
    call, within the budget, with rows.npy naming the reactors kept. float64 throughout; the clock columns
    of the stats are left out."""
    import torch
    import bench
    fields = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "cyc_total", "cyc_rhs",
              "cyc_jac", "cyc_lu", "cyc_sol", "t_end", "cyc_ctl", "cyc_clk", "t_ign", "ign_rate", "ign_dt", "nfe_dq")
    rng = np.random.default_rng(3)
    N, n = 1000, 9
    U = rng.random((N, n))
    st = rng.random((N, len(fields)))
    cols = [fields.index(k) for k in bench.DUMP_STATS]
    assert not any(k.startswith("cyc_") for k in bench.DUMP_STATS)

    info = bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(U), torch.from_numpy(st), fields)
    assert info["rows"] == N == info["of"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["U", "rows", "stats"] and all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["U"], U)
    np.testing.assert_array_equal(got["stats"], st[:, cols])
    np.testing.assert_array_equal(got["rows"], np.arange(N))

    budget = 40000
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    bench.dump_outputs(str(tmp_path / "b"), torch.from_numpy(U), torch.from_numpy(st), fields)
    bench.dump_outputs(str(tmp_path / "c"), torch.from_numpy(U), torch.from_numpy(st), fields)
    size = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert size <= budget
    rows = np.load(tmp_path / "b" / "rows.npy")
    k = len(rows)
    assert 0.8 * budget <= size and k < N and np.all(np.diff(rows) > 0)
    idx = rows.astype(int)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "U.npy"), U[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "stats.npy"), st[idx][:, cols])
    for f in ("U.npy", "stats.npy", "rows.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


def test_default_dump_budget_is_below_64_mb():
    import bench
    assert bench.DUMP_BYTES <= 64 * 10**6


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_timed_outputs(pkg, gpu, tmp_path):
    """One plain bench run on a small H2/O2 ensemble: the line reports the --steps it timed and none of
    the --full legs, and U.npy / stats.npy equal a direct Engine.integrate of the same seeded inputs
    (same kernel, same inputs: bit for bit)."""
    import bench
    from batchreactor_amd import ensemble
    N = 3000
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "h2o2", "--n", str(N), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "reactors/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - (N - line["solver"]["failed_all_ranks"]) / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["full"] is False
    assert line["cpu_baseline"] is None and line["parity_vs_oracle"] is None and line["value_incl_h2d_d2h"] is None
    assert "rate_jacobian" not in line["roofline"]
    assert line["outputs"]["rows"] == N

    m = bench.make_mech(pkg, "h2o2")
    T, Asv, U0 = ensemble.make_inputs(m, "h2o2", 0, N)
    eng = pkg.Engine(m, device=0)
    U, st = eng.integrate(T, Asv, U0, bench.CONFIGS["h2o2"]["tf"])
    eng.close()
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "rows.npy"), np.arange(N))
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "U.npy"), U)
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "stats.npy"),
                                  np.stack([st[k] for k in bench.DUMP_STATS], axis=1))
