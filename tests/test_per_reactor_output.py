"""Per-reactor output times (br_opts.tout_per_reactor: tout[N][nout], NaN = no output as trailing
padding) and ignition-phase sampling (br_phase_tout_dev, br_integrate_phase) in every engine.

The step sequence of a reactor does not depend on its outputs, and a reactor's arithmetic does not
depend on its neighbours, so the per-reactor mode is checked bit for bit: every yout row must equal the
row of a shared-grid run of the same grid, and u and the solver counters those of a run without
outputs. The odd ensemble sizes leave a partly filled last wave or group and put reactors with
different grids (different trip counts of the output loop) into one wave.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import LIB, ROOT
from parity_bands import OUT_T
from test_gpu_parity import _ignition_inputs, _mechs, close_states

TAU = (0.5, 0.8, 0.9, 0.95, 1.0, 1.05, 1.1, 1.5, 2.0, 10.0)
FRONT = np.array([0.8 < t < 2.0 for t in TAU])
COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "t_end", "t_ign", "ign_rate",
            "ign_dt", "nfe_dq")                       # every br_stats field except the cyc_* clocks

# engine (BRHIP_ENGINE, None = the mechanism's default), case, N
ENGINES = {"quad": (None, "h2o2", 37), "lane": ("lane", "h2o2", 70), "pair": ("pair", "surf", 13),
           "wave": ("wave", "gri", 9), "wave2": ("wave", "gas_surf", 5)}
KERNELS = {"quad": "k_group<16, 9>", "lane": "k_lane<9>", "pair": "k_group<32, 24>", "wave": "k_integrate<56>",
           "wave2": "k_integrate<72>"}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _engine(pkg, monkeypatch, which):
    from batchreactor_amd import ensemble
    env, case, N = ENGINES[which]
    if env is None:
        monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    else:
        monkeypatch.setenv("BRHIP_ENGINE", env)
    c = {"h2o2": dict(gas_mech="h2o2.dat"), "gri": dict(gas_mech="grimech.dat"),
         "surf": dict(surface_mech="ch4ni.xml", gasphase=["CH4", "H2O", "H2", "CO", "CO2", "O2", "N2"]),
         "gas_surf": dict(gas_mech="grimech.dat", surface_mech="ch4ni.xml")}[case]
    pm = pkg.Mechanism.from_files(LIB, **c)
    eng = pkg.Engine(pm)
    assert eng.kernel_name == KERNELS[which], eng.kernel_name
    T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    return pm, eng, T, Asv, U0, N


def _three_grids(t_med):
    """G0: the 28 shared output times of the parity tests. G1: starts at t <= 0 (u0 rows), a repeated
    interior time, an entry past every tf, two trailing NaNs. G2: 28 points in [0.5, 2] x the ensemble's
    median ignition time. All of length 28."""
    g0 = np.array(OUT_T)
    g1 = np.concatenate([[-1.0, 0.0, 0.0], np.logspace(-6, 0, 10), [1.0], np.logspace(0.1, 0.9, 11), [20.0],
                         [np.nan, np.nan]])
    g2 = np.linspace(0.5, 2.0, 28) * t_med
    assert len(g0) == len(g1) == len(g2) == 28 and np.all(np.diff(g1[:-2]) >= 0) and np.any(np.diff(g1[:-2]) == 0)
    return [g0, g1, g2]


def _mixed(grids, N):
    return np.stack([grids[i % 3] for i in range(N)])


# ------------------------------------------------------------------------------------ CPU
def test_phase_grid_properties(pkg):
    rng = np.random.default_rng(3)
    N = 50
    t_ign = np.exp(rng.uniform(np.log(1e-6), np.log(1.0), N))
    t_ign[[4, 17]] = np.nan
    tf = np.where(np.arange(N) % 2 == 0, 10.0, 1.2 * np.nan_to_num(t_ign, nan=1.0))
    tau = np.array(TAU)
    G = pkg.phase_grid(t_ign, tau, tf)
    assert G.shape == (N, len(tau)) and G.dtype == np.float64
    for i in range(N):
        fin = np.isfinite(G[i])
        k = int(fin.sum())
        assert np.all(fin[:k]) and not np.any(fin[k:]), (i, G[i])          # NaN only trailing
        assert np.all(np.diff(G[i, :k]) > 0)                               # ascending
        for j in range(len(tau)):
            p = tau[j] * t_ign[i]
            if t_ign[i] != t_ign[i] or p > tf[i]:
                assert G[i, j] != G[i, j], (i, j)
            else:
                assert G[i, j] == p, (i, j)                                # exactly the rounded product
    assert np.all(np.isnan(G[4])) and np.all(np.isnan(G[17]))
    assert np.isfinite(G[1, 6]) and np.isnan(G[1, 7])                      # tf = 1.2 t_ign: tau 1.1 kept, 1.5 dropped
    assert pkg.phase_grid(2.0, tau, 1e9).shape == (1, len(tau))            # scalars broadcast


def test_opts_field_and_symbols_in_every_binding(pkg):
    from test_julia_binding import _header, _julia
    _, structs, protos = _header()
    assert structs["br_opts"][-1] == ("tout_per_reactor", "int", [])
    assert pkg._lib.Opts._fields_[-1] == ("tout_per_reactor", C.c_int)
    assert [n for n, _, _ in structs["br_opts"]] == [f[0] for f in pkg._lib.Opts._fields_]
    _, src, calls, jstructs, _ = _julia()
    assert jstructs["BrOpts"][-1] == ("tout_per_reactor", "Cint")
    assert [n for n, _, _ in structs["br_opts"]] == [n for n, _ in jstructs["BrOpts"]]
    assert "tout_per_reactor" in src.split("\nBrOpts(;")[1].split(") =")[0]       # constructor keyword
    bound_jl = {c[0] for c in calls}
    for sym, nargs in (("br_phase_tout_dev", 7), ("br_integrate_phase", 12)):
        assert sym in protos and len(protos[sym][1]) == nargs, sym
        assert sym in pkg._lib.EXPORTS and sym in bound_jl, sym
    assert "function integrate_phase!(" in src
    assert "phase=nothing" in src.split("function batch_reactor_ensemble(")[1].split(")\n")[0]
    assert o_default(pkg).tout_per_reactor == 0


def o_default(pkg):
    e = pkg.Engine.__new__(pkg.Engine)
    e.device, e.ign1 = 0, 0
    return e._opts(1e-6, 1e-10, 100)


def test_wrong_tout_shape_raises_before_the_library(pkg, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    e = pkg.Engine.__new__(pkg.Engine)                 # no handle: nothing here may reach the GPU
    e.device, e.ign1, e.n, e.h = 0, 0, 9, None
    U0 = np.ones((5, 9))
    for bad in (np.zeros((4, 3)), np.zeros((6, 3)), np.zeros((5, 3, 2)), np.zeros((1, 3))):
        with pytest.raises(ValueError, match="tout"):
            e.integrate(np.full(5, 1000.0), np.ones(5), U0, 1.0, tout=bad)
        with pytest.raises(ValueError, match="tout"):
            pkg.integrate_multi([e, e], np.full(5, 1000.0), np.ones(5), U0, 1.0, tout=bad)
    to, per = pkg.engine.output_grid(np.zeros((5, 3)), 5)
    assert per and to.shape == (5, 3) and to.flags.c_contiguous
    to, per = pkg.engine.output_grid([0.0, 1.0], 5)
    assert not per and to.shape == (2,)
    assert pkg.engine.output_grid(None, 5) == (None, False)


def test_phase_parity_script_dry_run(tmp_path, orc):
    """scripts/phase_parity.py --cpu-dry-run (a jittered oracle stands in for the GPU): a well-formed
    JSON, every phase scored, the oracle's self-spread and the marker's resolution recorded."""
    out = tmp_path / "pp.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "phase_parity.py"), "--cpu-dry-run", "--configs",
                        "h2o2,surf", "--sample", "8", "--threads", "4", "--no-converged-front", "--out", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(out.read_text())
    assert d["tau"] == list(TAU)
    assert "skipped" in d["configs"]["surf"]
    for jac in ("analytic", "dq"):
        c = d["configs"]["h2o2"][jac]
        assert c["sample"] == 8 and c["scored"] == 8 and c["eps_cal"] > 0
        for key in ("gpu_vs_oracle", "oracle_self_spread"):
            assert [p["tau"] for p in c[key]] == list(TAU)
            assert all(p["reactors"] == 8 and p["max"] >= p["median"] >= 0 for p in c[key])
        pr = c["per_reactor"]
        assert all(len(pr[k]) == 8 for k in ("t_ign_gpu", "t_ign_orc", "t_ign_rel_diff", "ign_dt_over_t_ign_gpu",
                                             "ign_dt_over_t_ign_orc"))
        assert all(0 < v < 1 for v in pr["ign_dt_over_t_ign_orc"])
        assert c["t_ign_rel_diff"]["max"] >= c["t_ign_rel_diff"]["median"] >= 0


# the front bounds of test_converged_front_against_oracle, (case, dq) -> (raw maximum, bound = 4 x raw): the
# oracle's own convergence error at the front phases, derived on the CPU (see that test)
_RAW_FRONT = {("gri", False): 8.694, ("gri", True): 12.005, ("h2o2", False): 0.7062, ("h2o2", True): 0.6033}
CONVERGED_FRONT = {k: (raw, 4 * raw) for k, raw in _RAW_FRONT.items()}


def test_converged_front_bounds_are_the_committed_derivation():
    d = json.load(open(os.path.join(ROOT, "profiles", "phase_parity.json")))["converged_front"]
    assert d["tau"] == list(TAU) and d["reactors"] == 16
    for (case, dq), (raw, bound) in CONVERGED_FRONT.items():
        c = d["cases"][case]["dq" if dq else "analytic"]
        assert bound == 4 * raw
        assert abs(c["raw_max"] / raw - 1) < 5e-3 and abs(c["bound"] / bound - 1) < 5e-3, (case, dq, c)


# ------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("which", list(ENGINES))
def test_per_reactor_grids_bit_exact_against_shared(pkg, gpu, monkeypatch, which):
    """Reactor i gets grid G[i % 3] (_three_grids), tf alternates between 10 s and 2e-3 s: every yout
    row equals the row of the shared-grid run of that grid (np.array_equal), rows of NaN entries and
    of times past tf stay 0.0, and u and every counter equal a run without outputs."""
    pm, eng, T, Asv, U0, N = _engine(pkg, monkeypatch, which)
    tf = np.where(np.arange(N) % 2 == 0, 10.0, 2e-3)
    Up, sp = eng.integrate(T, Asv, U0, tf)
    t_med = np.nanmedian(sp["t_ign"]) if np.any(np.isfinite(sp["t_ign"])) else 1e-3   # (surface-only: no marker)
    grids = _three_grids(t_med)
    tout = _mixed(grids, N)
    U, st = eng.integrate(T, Asv, U0, tf, tout=tout)
    assert np.array_equal(U, Up)
    for k in COUNTERS:
        assert _same(st[k], sp[k]), k
    Y = st["yout"]
    assert Y.shape == (N, 28, pm.n)
    written = 0
    for g, grid in enumerate(grids):
        fin = np.isfinite(grid)
        Us, ss = eng.integrate(T, Asv, U0, tf, tout=grid[fin])
        assert np.array_equal(Us, Up)
        for i in range(g, N, 3):
            assert np.array_equal(Y[i][fin], ss["yout"][i]), (which, g, i)
            assert np.all(Y[i][~fin] == 0.0), (which, g, i)
            past = fin & (np.nan_to_num(grid, nan=np.inf) > tf[i])
            assert np.all(Y[i][past] == 0.0)
            written += int(np.any(Y[i][fin & ~past] != 0.0, axis=1).sum())
        if g == 1:
            for i in range(1, N, 3):
                assert np.array_equal(Y[i][0], U0[i]) and np.array_equal(Y[i][2], U0[i])   # t <= 0: u0
    assert written > 10 * N          # (the comparison is not one of empty rows)


# Front bounds, derived on the CPU (scripts/phase_parity.py --converged-front-only, committed under
# "converged_front" in profiles/phase_parity.json): close_states(rtol 1e-6, floor 1e-14) of the oracle at
# rtol 1e-10 / atol 1e-16 against the oracle at rtol 1e-11 / atol 1e-17, same 16 reactors, at tau * t_ign.
@pytest.mark.gpu
@pytest.mark.parametrize("case,dq", [("gri", False), ("gri", True), ("h2o2", False), ("h2o2", True)],
                         ids=["gri", "gri-dq", "h2o2", "h2o2-dq"])
def test_converged_front_against_oracle(pkg, orc, gpu, case, dq):
    """Tight tolerances on both sides (rtol 1e-10, atol 1e-16, tf = 1e-2, the inputs of
    test_integrate_parity_tight, 16 reactors): the GPU at the ten phases TAU x its own t_ign (a
    per-reactor grid), the oracle at the same times. close_states(rtol 1e-6, floor 1e-14) <= 1 at the
    phases <= 0.8 and >= 2; at the front phases (0.9 .. 1.5) <= the bound CONVERGED_FRONT[(case, dq)]
    = 4 x the oracle's own convergence error there (rtol 1e-10 against rtol 1e-11; two sides each carry
    it, times the margin of 2 of parity_bands.py). Raw maxima -> bounds: GRI analytic 8.694 -> 34.78, GRI DQ
    12.005 -> 48.02, H2/O2 analytic 0.7062 -> 2.825, H2/O2 DQ 0.6033 -> 2.413 (the GRI maximum is at tau =
    1, where the marker sits inside the steepest step; the other front phases are below 0.6). Never
    derived from a GPU run."""
    from concurrent.futures import ThreadPoolExecutor
    N, tf = 16, 1e-2
    pm, om = _mechs(pkg, orc, case)
    eng = pkg.Engine(pm)
    T, Asv, U0 = _ignition_inputs(pm, case, N, 6)
    _, s0 = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
    assert np.all(s0["status"] == 0) and np.all(np.isfinite(s0["t_ign"]))
    grid = pkg.phase_grid(s0["t_ign"], TAU, tf)
    _, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq, tout=grid)
    assert _same(st["t_ign"], s0["t_ign"])

    def oracle(i):
        sel = np.isfinite(grid[i])
        _, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], tf, grid[i][sel], rtol=1e-10, atol=1e-16, analytic_jac=not dq)
        assert so["status"] == 0
        return np.array([close_states(st["yout"][i][sel][j], Yo[j], rtol=1e-6, floor=1e-14) if s else np.nan
                         for j, s in zip(np.cumsum(sel) - 1, sel)])

    with ThreadPoolExecutor(8) as ex:
        E = np.array(list(ex.map(oracle, range(N))))
    with np.errstate(all="ignore"):
        worst = np.nanmax(E, axis=0)
    raw, bound = CONVERGED_FRONT[(case, dq)]
    print(f"\n  {case}{' (DQ)' if dq else ''}: close_states per phase {np.round(worst, 4)}; front bound {bound:.4g}")
    assert np.isfinite(E[:, :5]).all()                 # every reactor ignites well inside tf: phases <= 1 exist
    for j, tau in enumerate(TAU):
        e = E[:, j][np.isfinite(E[:, j])]
        if len(e):
            assert e.max() <= (bound if FRONT[j] else 1.0), (case, dq, tau, e.max())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["quad", "wave"])
def test_phase_sampling(pkg, gpu, monkeypatch, which):
    """integrate_phase: t_ign, u and the counters bit-equal to a plain run's; stats["tout"] exactly
    phase_grid(t_ign, tau, tf); stats["yout"] exactly what integrate(tout=that grid) gives; a reactor
    with tf = 1.2 t_ign has its tau >= 1.5 entries NaN and those yout rows untouched; without the
    ignition marker BR_ERR_INPUT."""
    pm, eng, T, Asv, U0, N = _engine(pkg, monkeypatch, which)
    _, s0 = eng.integrate(T, Asv, U0, 10.0)
    tf = np.full(N, 10.0)
    k = 2
    tf[k] = 1.2 * s0["t_ign"][k]
    Up, sp = eng.integrate(T, Asv, U0, tf)
    assert np.all(sp["status"] == 0) and np.all(np.isfinite(sp["t_ign"]))
    U, st = eng.integrate_phase(T, Asv, U0, tf, TAU)
    assert np.array_equal(U, Up)
    for key in COUNTERS:
        assert _same(st[key], sp[key]), key
    grid = pkg.phase_grid(sp["t_ign"], TAU, tf)
    assert _same(st["tout"], grid)
    assert np.all(np.isfinite(grid[k][:7])) and np.all(np.isnan(grid[k][7:9]))       # tau 1.5, 2 past tf
    assert np.all(st["yout"][np.isnan(grid)] == 0.0)
    assert np.all(np.any(st["yout"][np.isfinite(grid)] != 0.0, axis=1))
    _, s2 = eng.integrate(T, Asv, U0, tf, tout=grid)
    assert np.array_equal(st["yout"], s2["yout"])
    eng.ign1 = 0
    with pytest.raises(RuntimeError, match="-10"):
        eng.integrate_phase(T, Asv, U0, tf, TAU)


@pytest.mark.gpu
def test_per_reactor_grids_multi_handle(pkg, gpu, monkeypatch):
    """br_integrate_multi slices a 2-D tout with the ensemble: two handles give exactly the
    single-handle result (N = 37: slices of 19 and 18, neither a multiple of 3)."""
    pm, eng, T, Asv, U0, N = _engine(pkg, monkeypatch, "quad")
    tf = np.where(np.arange(N) % 2 == 0, 10.0, 2e-3)
    tout = _mixed(_three_grids(1e-4), N)
    U1, s1 = eng.integrate(T, Asv, U0, tf, tout=tout)
    engines = [pkg.Engine(pm, device=0) for _ in range(2)]
    Um, sm = pkg.integrate_multi(engines, T, Asv, U0, tf, tout=tout)
    assert np.array_equal(U1, Um) and np.array_equal(s1["yout"], sm["yout"])
    assert np.any(s1["yout"][19:] != 0.0)
    for key in COUNTERS:
        assert _same(s1[key], sm[key]), key


@pytest.mark.gpu
def test_phase_tout_device(pkg, gpu, monkeypatch):
    """br_phase_tout_dev on torch tensors equals phase_grid exactly, NaN positions included; and the
    device-resident two-pass flow (integrate_device, phase_tout_device, integrate_device with the
    per-reactor device grid) gives integrate_phase's outputs."""
    import torch
    pm, eng, T, Asv, U0, N = _engine(pkg, monkeypatch, "quad")
    dev = torch.device("cuda", 0)
    tf = np.full(N, 10.0)
    dT, dA, dtf = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (T, Asv, tf))
    dU = torch.from_numpy(U0).to(dev)
    dst = torch.zeros((N, pkg._lib.NSTAT), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    eng.integrate_device(dT.data_ptr(), dA.data_ptr(), dU.data_ptr(), dtf.data_ptr(), dst.data_ptr(), N, stream)
    torch.cuda.synchronize()
    t_ign = dst[:, 16].cpu().numpy().copy()
    # synthetic cases on top of the integrated ones: an unknown t_ign, a tf that cuts the row
    dst2 = dst.clone()
    dst2[5, 16] = float("nan")
    tf2 = tf.copy()
    tf2[7] = 1.2 * t_ign[7]
    t2 = t_ign.copy()
    t2[5] = np.nan
    dtau = torch.tensor(TAU, dtype=torch.float64, device=dev)
    G = eng.phase_tout_device(dst2, dtau, torch.from_numpy(tf2).to(dev))
    torch.cuda.synchronize()
    ref = pkg.phase_grid(t2, TAU, tf2)
    Gh = G.cpu().numpy()
    assert np.array_equal(np.isnan(Gh), np.isnan(ref)) and _same(Gh, ref)
    assert np.all(np.isnan(Gh[5])) and np.isnan(Gh[7, 7]) and np.isfinite(Gh[7, 6])
    with pytest.raises(ValueError):
        eng.phase_tout_device(dst2[:, :5], dtau, dtf)
    # pass 2 on the device with the grid of the unmodified first pass
    G1 = eng.phase_tout_device(dst, dtau, dtf)
    dU.copy_(torch.from_numpy(U0).to(dev))
    dY = torch.zeros((N, len(TAU), pm.n), dtype=torch.float64, device=dev)
    eng.integrate_device(dT.data_ptr(), dA.data_ptr(), dU.data_ptr(), dtf.data_ptr(), dst.data_ptr(), N, stream,
                         tout_ptr=G1.data_ptr(), yout_ptr=dY.data_ptr(), nout=len(TAU), tout_per_reactor=True)
    torch.cuda.synchronize()
    U, st = eng.integrate_phase(T, Asv, U0, tf, TAU)
    assert _same(G1.cpu().numpy(), st["tout"])
    assert np.array_equal(dY.cpu().numpy(), st["yout"]) and np.array_equal(dU.cpu().numpy(), U)


@pytest.mark.gpu
def test_per_reactor_grid_input_errors(pkg, gpu, monkeypatch):
    """A descending row and a NaN before a number, each in row 1 of 3, give BR_ERR_INPUT with the
    reactor's index in br_last_error(); the rows are checked on the host, before any launch: the fresh
    handle has still recorded no kernel afterwards."""
    pm, eng, T, Asv, U0, N = _engine(pkg, monkeypatch, "quad")
    other = pkg.Engine(pm)
    T, Asv, U0, N = T[:3], Asv[:3], U0[:3], 3
    good = np.array([1e-5, 1e-4, 1e-3, np.nan])
    for bad, what in ((np.array([1e-5, 1e-3, 1e-4, np.nan]), "ascending"), (np.array([1e-5, np.nan, 1e-3, np.nan]), "NaN")):
        tout = np.stack([good, bad, good])
        with pytest.raises(RuntimeError, match=r"-10.*reactor 1\b") as ei:
            eng.integrate(T, Asv, U0, 1e-2, tout=tout)
        assert what in str(ei.value)
        with pytest.raises(RuntimeError, match=r"-10.*reactor 1\b"):
            pkg.integrate_multi([eng, other], T, Asv, U0, 1e-2, tout=tout)
        for e in (eng, other):
            with pytest.raises(RuntimeError, match="no kernel recorded"):
                e.last_kernel_ms()
    U, st = eng.integrate(T, Asv, U0, 1e-2, tout=np.stack([good, good, good]))     # (the good rows pass)
    assert np.all(st["status"] == 0) and np.all(st["yout"][:, 3] == 0.0) and np.all(st["yout"][:, 2, 0] != 0.0)
