"""Adiabatic constant-volume reactors on the group engines (k_group<GL, NM, true>; BRHIP_ENGINE = quad / pair), on
the GPU: trajectories against the CPU statement inside that statement's own spread, converged runs against SciPy's
Radau with the conservation of E and of mass, the bitwise identities of a batched run (a reactor's arithmetic does
not depend on its wave neighbours), slot reuse inside one launch, the plumbing of the other entry points, and the
default path, which has not moved. The bounds are test_energy_gpu.py's."""
import numpy as np
import pytest

import energy_cases as ec
import energy_group_cases as egc
from test_gpu_parity import close_states

pytestmark = pytest.mark.gpu

COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "nfe_dq")
TIMES = ("t_end", "t_ign", "ign_dt", "ign_rate")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _same_runs(U, st, V, sv, what, keys=COUNTERS + TIMES + ("T_end",)):
    assert _same(U, V), what
    for k in keys:
        assert _same(st[k], sv[k]), (what, k)


def _five(pm, name="h2o2"):
    """five different reactors: the regime's mixture at five initial temperatures (test_energy_gpu._five's), on pm"""
    r = ec.REGIMES[name]
    T = r["T0"] + np.array([0.0, 40.0, -30.0, 90.0, 150.0])
    U0 = np.stack([pm.initial_state(Ti, r["p"], pm.mole_fractions(r["x"])) for Ti in T])
    return T, np.ones(5), U0, np.full(5, r["tf"])


def _expect_engine(eng, gl, nm):
    assert eng.energy_launch_info()["engine"] == -(100 * gl + nm), eng.energy_launch_info()


# --------------------------------------------------------------------------------- 1. trajectories
@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
def test_trajectory_against_the_cpu_statement(pkg, orc, gpu, monkeypatch, conv):
    """test_energy_gpu's test of the same name on the quad energy instance, H2/O2: yout and T_out at 28 of the host
    run's accepted steps and at tf, per ignition window within max(2 x the CPU statement's own spread, 1e-6); t_ign
    within max(ign_dt of either run, 2 x that spread in t_ign); the step count within 35 %; nfe_dq == nje (ng + 1).
    The host spread is what a last-bit perturbation does to this trajectory; the group sums' order is one."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    name = "h2o2"
    pm, om, y0, tf = ec.mechs(pkg, orc, name, conv)
    base = ec.host_run(pkg, orc, name, conv)
    spread, dt_spread = ec.host_spread(pkg, orc, name, conv)
    bound = np.maximum(2.0 * spread, 1e-6)
    pk = ec.picks(base)
    tq = base["t"][pk]
    eng = pkg.Engine(pm)
    _expect_engine(eng, 16, 16)
    U, st = eng.integrate([y0[-1]], [1.0], y0[None, :-1], [tf], tout=tq, energy="adiabatic")
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * (pm.ng + 1) and st["nje"][0] > 0
    Yg = np.concatenate([st["yout"][0], st["T_out"][0][:, None]], axis=1)
    e = ec.window_errors(Yg, base["Y"][pk], base["t_ign"], tq)
    e = np.maximum(e, ec.window_errors(np.append(U[0], st["T_end"][0]), base["y"], base["t_ign"], [tf]))
    d_ign = abs(st["t_ign"][0] - base["t_ign"])
    b_ign = max(st["ign_dt"][0], base["ign_dt"], 2.0 * dt_spread)
    print(f"\n  quad {name} conv {conv}: bands pre / front / post {e[0]:.3g} / {e[1]:.3g} / {e[2]:.3g}, host spread "
          f"{spread[0]:.3g} / {spread[1]:.3g} / {spread[2]:.3g}; t_ign {st['t_ign'][0]:.6g} vs {base['t_ign']:.6g} "
          f"(bound {b_ign:.3g}, host spread {dt_spread:.3g}); T_end {st['T_end'][0]:.2f} vs {base['y'][-1]:.2f}; "
          f"steps {int(st['nsteps'][0])} vs {int(base['stats'][0])}")
    assert np.all(e <= bound), (name, conv, e, bound)
    assert d_ign <= b_ign, (name, conv, d_ign, b_ign)
    assert abs(st["nsteps"][0] - base["stats"][0]) <= 0.35 * base["stats"][0]
    assert _same(st["T_out"][0][-1], st["T_end"][0]) or tq[-1] != tf
    eng.close()


# --------------------------------------------------------------------------------- 2. converged, conservation
def _converged(eng, pm, y0, tf, ref, host, what):
    """rtol 1e-10 / atol 1e-16 with 28 outputs at the host run's steps: the end state and T_end against ref to 1e-6
    relative (floor 1e-14), E drift <= max(4 x the host run's, 1e-12), sum_k u_k constant to 1e-12"""
    tq = host["t"][ec.picks(host)]
    U, st = eng.integrate([y0[-1]], [1.0], y0[None, :-1], [tf], rtol=1e-10, atol=1e-16, tout=tq, energy="adiabatic")
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * (pm.ng + 1) and st["nje"][0] > 0
    e = close_states(np.append(U[0], st["T_end"][0]), ref, rtol=1e-6, floor=1e-14)
    E0 = pm.internal_energy(y0[:-1], y0[-1])
    E = np.append(pm.internal_energy(st["yout"][0], st["T_out"][0]), pm.internal_energy(U[0], st["T_end"][0]))
    drift = float(np.max(np.abs(E / E0 - 1.0)))
    drift_host = float(np.max(np.abs(host["E"] / host["E"][0] - 1.0)))
    rho = np.append(st["yout"][0].sum(axis=1), U[0].sum())
    dm = float(np.max(np.abs(rho / y0[:-1].sum() - 1.0)))
    print(f"\n  {what}: converged error {e:.3g} of the 1e-6 bar, T_end {st['T_end'][0]:.2f} K; E drift {drift:.3g} "
          f"(host {drift_host:.3g}), mass drift {dm:.3g}")
    assert e <= 1.0, (what, e)
    assert drift <= max(4.0 * drift_host, 1e-12), (what, drift, drift_host)
    assert dm <= 1e-12, (what, dm)


def test_converged_h2o2_quad(pkg, orc, gpu, monkeypatch):
    """test_converged_against_radau_and_conservation's conditions on the quad energy instance <16, 16>, H2/O2"""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    pm, om, y0, tf = ec.mechs(pkg, orc, "h2o2", 0)
    eng = pkg.Engine(pm)
    _expect_engine(eng, 16, 16)
    _converged(eng, pm, y0, tf, ec.radau_end(pkg, orc, "h2o2"), ec.host_run(pkg, orc, "h2o2", 0, rtol=1e-10, atol=1e-16),
               "quad h2o2")
    eng.close()


@pytest.mark.parametrize("key,engine,gl,nm", [("s8", "quad", 16, 9), ("s24", "pair", 32, 32)])
def test_converged_written_mechanisms(pkg, orc, gpu, monkeypatch, tmp_path_factory, key, engine, gl, nm):
    """... on <16, 9> (S8: H2/O2 without N2, {H2 .6, O2 .4}, 1100 K, tf 1e-3) and <32, 32> (S24: 129 reactions with
    Troe falloff, {CH4 .1, O2 .2, N2 .7}, 1500 K, tf 5e-3), each against its own Radau reference and host drift"""
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    pm, om, y0, tf = egc.regime(pkg, orc, tmp_path_factory, key, 0)
    eng = pkg.Engine(pm)
    _expect_engine(eng, gl, nm)
    _converged(eng, pm, y0, tf, egc.radau_end(pkg, orc, tmp_path_factory, key),
               egc.host_run(pkg, orc, tmp_path_factory, key, 0, rtol=1e-10, atol=1e-16), f"{engine} {key}")
    eng.close()


@pytest.mark.parametrize("n,engine,gl,nm", [(15, "quad", 16, 16), (16, "pair", 32, 24), (31, "pair", 32, 32)])
def test_converged_at_the_width_boundaries(pkg, orc, gpu, monkeypatch, tmp_path_factory, n, engine, gl, nm):
    """H2/O2 with inert species at zero concentration up to ng = 15 (T on the last lane of a 16-lane group), 16 (the
    pair instance <32, 24>, one shape up from the isothermal <16, 16>) and 31 (T on lane 31): the same ODE as the
    nine-species regime. At rtol 1e-10 / atol 1e-16 the shared species and T_end agree with its Radau reference to
    1e-6 (floor 1e-14), the inerts stay 0 to that floor (test_energy_gpu's test of the same name says why not
    exactly)."""
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    pm9, _, y9, tf = ec.mechs(pkg, orc, "h2o2", 0)
    ref = ec.radau_end(pkg, orc, "h2o2")
    pm, _ = egc.written(pkg, orc, tmp_path_factory, f"h2o2_n{n}", 0)
    assert pm.ng == n and pm.gas_species[:9] == pm9.gas_species
    r = ec.REGIMES["h2o2"]
    u0 = pm.initial_state(r["T0"], r["p"], pm.mole_fractions(r["x"]))
    assert np.array_equal(u0[:9], y9[:-1]) and not u0[9:].any()
    eng = pkg.Engine(pm)
    _expect_engine(eng, gl, nm)
    U, st = eng.integrate([r["T0"]], [1.0], u0[None, :], [tf], rtol=1e-10, atol=1e-16, energy="adiabatic")
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * (n + 1) and np.all(np.abs(U[0, 9:]) <= 1e-14)
    e = close_states(np.append(U[0, :9], st["T_end"][0]), ref, rtol=1e-6, floor=1e-14)
    print(f"\n  {engine} ng = {n}: converged error {e:.3g} of the 1e-6 bar, T_end {st['T_end'][0]:.2f} K")
    assert e <= 1.0, (n, e)
    eng.close()


# --------------------------------------------------------------------------------- 3. bitwise identities
@pytest.mark.parametrize("engine", ["quad", "pair"])
def test_bitwise_identities(pkg, orc, gpu, monkeypatch, tmp_path_factory, engine):
    """Five different reactors integrated together (two waves' groups, diverging) equal the same five one at a time;
    a run with tout equals the run without; multipliers all 1.0 equal no multipliers: in U, T_end and every counter
    and time, bit for bit. quad: H2/O2; pair: the same five with inert species up to ng = 16."""
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    pm = ec.mechs(pkg, orc, "h2o2", 0)[0] if engine == "quad" else egc.written(pkg, orc, tmp_path_factory, "h2o2_n16", 0)[0]
    T, Asv, U0, tf = _five(pm)
    eng = pkg.Engine(pm)
    _expect_engine(eng, *((16, 16) if engine == "quad" else (32, 24)))
    U, st = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    assert np.all(st["status"] == 0) and np.ptp(st["T_end"]) > 10.0 and np.all(st["T_end"] > T + 500.0)
    assert np.all(st["nfe_dq"] == st["nje"] * (pm.ng + 1))
    for i in range(5):
        Ui, si = eng.integrate(T[i:i + 1], Asv[i:i + 1], U0[i:i + 1], tf[i:i + 1], energy="adiabatic")
        assert _same(Ui[0], U[i]) and _same(si["T_end"][0], st["T_end"][i]), i
        for k in COUNTERS + TIMES:
            assert _same(si[k][0], st[k][i]), (i, k)
    variants = {"tout": dict(tout=np.array([0.0, 1e-6, 5e-5, 2e-4, 1e-3])),
                "ones": dict(rate_mult=np.ones((1, eng.nr)), rate_mult_row=np.zeros(5, np.int32))}
    for what, kw in variants.items():
        Uv, sv = eng.integrate(T, Asv, U0, tf, energy="adiabatic", **kw)
        _same_runs(U, st, Uv, sv, what)
        if what == "tout":                      # outputs: u0 / T0 at t = 0 (written before the first step), the end state at tf
            assert _same(sv["T_out"][:, 0], T) and _same(sv["yout"][:, 0], U0)
            assert _same(sv["T_out"][:, -1], st["T_end"]) and _same(sv["yout"][:, -1], U)
            assert np.all(np.diff(sv["T_out"], axis=1) >= -1e-6)
    eng.close()


# --------------------------------------------------------------------------------- 4. slot reuse
def test_slot_reuse_inside_one_launch(pkg, orc, gpu, monkeypatch):
    """More reactors than the persistent grid holds at once (resident + 37), all with bitwise the same T(0) = 1100 K
    and u0, their multiplier rows cycling through (all 1.0; reaction 0 x 1.5; reaction 3 x 0.5): every group takes
    further reactors in the slot of its first, whose T(0) is the cached T of its predecessor but whose constants
    are not. Each reactor equals, bit for bit in U, T_end, counters and times, the reactor of its row in a
    3-reactor run."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    pm, _, y0, _ = ec.mechs(pkg, orc, "h2o2", 0)
    eng = pkg.Engine(pm)
    info = eng.energy_launch_info()
    assert info["engine"] == -1616 and info["resident"] >= info["reactors_per_workgroup"]
    N = info["resident"] + 37
    tab = np.ones((3, eng.nr))
    tab[1, 0], tab[2, 3] = 1.5, 0.5
    tf = 2e-4

    def run(n, rows):
        return eng.integrate(np.full(n, 1100.0), np.ones(n), np.tile(y0[:-1], (n, 1)), np.full(n, tf), rate_mult=tab,
                             rate_mult_row=rows.astype(np.int32), energy="adiabatic")
    U3, s3 = run(3, np.arange(3))
    assert np.all(s3["status"] == 0)
    assert not _same(U3[0], U3[1]) and not _same(U3[0], U3[2]) and not _same(U3[1], U3[2])   # (the rows do differ)
    rows = np.arange(N) % 3
    U, st = run(N, rows)
    bad = np.flatnonzero(np.any(U != U3[rows], axis=1) | (st["T_end"] != s3["T_end"][rows]))
    assert bad.size == 0, (N, bad[:10], rows[bad[:10]])
    for k in COUNTERS + TIMES:
        assert _same(st[k], s3[k][rows]), k
    eng.close()


# --------------------------------------------------------------------------------- 5. plumbing
def test_multi_phase_and_isothermal_after(pkg, orc, gpu, monkeypatch):
    """test_energy_gpu's test of the same name under BRHIP_ENGINE=quad: br_integrate_multi (two handles) equals the
    single call, T_end, T_out and yout sliced with the ensemble; integrate_phase puts T_out at tau x t_ign and
    equals a run on its grid; an isothermal run on the handle after the group energy runs (which resize the
    shared group workspace) is bitwise the one before them."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    pm = ec.mechs(pkg, orc, "h2o2", 0)[0]
    T, Asv, U0, tf = _five(pm)
    eng, e2 = pkg.Engine(pm), pkg.Engine(pm)
    _expect_engine(eng, 16, 16)
    assert eng.kernel_name == "k_group<16, 9>"                           # the isothermal runs: the quad engine too
    Ui0, si0 = eng.integrate(T, Asv, U0, tf, dq_jacobian=True)
    tout = np.array([2e-5, 1e-4, 1e-3])
    U, st = eng.integrate(T, Asv, U0, tf, tout=tout, energy="adiabatic")
    Um, sm = pkg.integrate_multi([eng, e2], T, Asv, U0, tf, tout=tout, energy="adiabatic")
    assert np.all(st["status"] == 0)
    _same_runs(U, st, Um, sm, "multi", COUNTERS + TIMES + ("T_end", "T_out", "yout"))
    tau = np.array([0.5, 1.0, 2.0])
    Up, sp = eng.integrate_phase(T, Asv, U0, tf, tau, energy="adiabatic")
    assert _same(Up, U) and _same(sp["t_ign"], st["t_ign"]) and _same(sp["T_end"], st["T_end"])
    assert _same(sp["tout"], pkg.phase_grid(st["t_ign"], tau, tf)) and np.all(np.isfinite(sp["tout"]))
    U2, s2 = eng.integrate(T, Asv, U0, tf, tout=sp["tout"], energy="adiabatic")
    assert _same(sp["T_out"], s2["T_out"]) and _same(sp["yout"], s2["yout"])
    assert np.all(sp["T_out"][:, 0] < sp["T_out"][:, 1]) and np.all(sp["T_out"][:, 1] < sp["T_out"][:, 2])   # T rises through the front
    Ui1, si1 = eng.integrate(T, Asv, U0, tf, dq_jacobian=True)
    _same_runs(Ui0, si0, Ui1, si1, "isothermal after", COUNTERS + TIMES)
    assert not _same(U, Ui0)
    eng.close()
    e2.close()


def test_sensitivity_is_the_quotient_of_explicit_runs(pkg, orc, gpu, monkeypatch):
    """test_energy_gpu's test of the same name under BRHIP_ENGINE=quad: sensitivity(energy="adiabatic") on 2 H2/O2
    reactors x 3 reactions equals the central difference of explicit rate_mult runs (the expanded reactors are those
    runs, on the same group energy instance): S_u to 1e-14 relative, S_tign to 1e-14 (|ln t+| + |ln t-|) / (2 ln f)."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    pm = ec.mechs(pkg, orc, "h2o2", 0)[0]
    T, Asv, U0, tf = (a[:2] for a in _five(pm))
    eng = pkg.Engine(pm)
    _expect_engine(eng, 16, 16)
    rx, f = np.array([0, 3, 8], np.int32), 1.5
    out = eng.sensitivity(T, Asv, U0, tf, factor=f, reactions=rx, states=True, energy="adiabatic")
    assert out["nbad"] == 0 and np.abs(out["S_tign"]).max() > 0.05
    den = 2.0 * np.log(f)
    for j, r in enumerate(rx):
        tab = np.ones((2, eng.nr))
        tab[0, r], tab[1, r] = f, 1.0 / f
        Up, sp = eng.integrate(T, Asv, U0, tf, rate_mult=tab, rate_mult_row=np.zeros(2, np.int32), energy="adiabatic")
        Um, sm = eng.integrate(T, Asv, U0, tf, rate_mult=tab, rate_mult_row=np.ones(2, np.int32), energy="adiabatic")
        assert np.all(sp["status"] == 0) and np.all(sm["status"] == 0)
        lp, lm = np.log(sp["t_ign"]), np.log(sm["t_ign"])
        assert np.all(np.abs(out["S_tign"][:, j] - (lp - lm) / den) <= 1e-14 * (np.abs(lp) + np.abs(lm)) / den), r
        np.testing.assert_allclose(out["S_u"][:, j], (Up - Um) / den, rtol=1e-14, atol=0.0)
    U, st = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    assert _same(out["u"], U) and _same(out["stats"]["t_ign"], st["t_ign"])
    eng.close()


# --------------------------------------------------------------------------------- 6. the default has not moved
def test_the_default_has_not_moved(pkg, orc, gpu, monkeypatch):
    """With BRHIP_ENGINE unset an energy run is the wavefront energy instance: bitwise the run under
    BRHIP_ENGINE=wave, energy_launch_info engine 0. Under quad the end states differ from it in the last bits at
    most (close_states at rtol 1e-4), with nfe_dq == nje * 10. GRI-Mech (ng + 1 = 54: no group energy instance)
    under quad runs, bitwise its wave run."""
    pm = ec.mechs(pkg, orc, "h2o2", 0)[0]
    T, Asv, U0, tf = _five(pm)
    eng = pkg.Engine(pm)
    monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    assert eng.energy_launch_info()["engine"] == 0 and eng.energy_kernel_name == "k_integrate<16, false, true>"
    Ud, sd = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    assert eng.energy_launch_info()["engine"] == 0
    Uw, sw = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    assert np.all(sd["status"] == 0)
    _same_runs(Ud, sd, Uw, sw, "unset vs wave")
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    _expect_engine(eng, 16, 16)
    Uq, sq = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    assert np.all(sq["status"] == 0) and np.all(sq["nfe_dq"] == sq["nje"] * 10) and np.all(sq["nje"] > 0)
    e = max(close_states(np.append(Uq[i], sq["T_end"][i]), np.append(Uw[i], sw["T_end"][i]), rtol=1e-4) for i in range(5))
    print(f"\n  quad vs wave, five H2/O2 reactors: {e:.3g} of close_states' rtol 1e-4 bar")
    assert e <= 1.0, e
    eng.close()
    gm, _, y0, _ = ec.mechs(pkg, orc, "gri", 0)
    eng = pkg.Engine(gm)
    runs = {}
    for env in ("quad", "wave"):
        monkeypatch.setenv("BRHIP_ENGINE", env)
        assert eng.energy_launch_info()["engine"] == 0
        runs[env] = eng.integrate([y0[-1]], [1.0], y0[None, :-1], [2e-4], energy="adiabatic")
    assert runs["quad"][1]["status"][0] == 0
    _same_runs(*runs["quad"], *runs["wave"], "gri quad vs wave")
    eng.close()
