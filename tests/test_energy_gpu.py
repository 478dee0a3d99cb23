"""Adiabatic constant-volume reactors in the wavefront engine (br_opts.energy), on the GPU: the energy
instances' right-hand side against oracle.rhs + Mechanism.thermo_e_cv, trajectories against the CPU statement
(br_integrate_host on f(t, [u, T]), tests/energy_cases.py) inside that statement's own spread, converged runs
against SciPy's Radau, conservation of E = sum_k c_k e_k(T) and of mass, the bitwise identities of a batched
run, and the plumbing of the other entry points."""
import os

import numpy as np
import pytest

import energy_cases as ec
from conftest import LIB
from test_gpu_parity import SURF_GAS, TH, _h2o2_with_inerts, _scale, _states, close_states
from test_group_kernels import S24, subset_mechanism

pytestmark = pytest.mark.gpu

COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "nfe_dq")
TIMES = ("t_end", "t_ign", "ign_dt", "ign_rate")
R_GAS = 8.31446261815324


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _five(pkg, orc, name="h2o2", conv=0):
    """five different reactors of a regime's mechanism: its mixture at five initial temperatures"""
    pm, om, y0, tf = ec.mechs(pkg, orc, name, conv)
    r = ec.REGIMES[name]
    T = r["T0"] + np.array([0.0, 40.0, -30.0, 90.0, 150.0])
    U0 = np.stack([pm.initial_state(Ti, r["p"], pm.mole_fractions(r["x"])) for Ti in T])
    return pm, T, np.ones(5), U0, np.full(5, tf)


# --------------------------------------------------------------------------------- 1. the right-hand side
def _eval_case(pkg, orc, tmp_path, mech, conv):
    if mech == "s24":
        d = subset_mechanism(tmp_path, S24, name="s24e")
        return (pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=conv),
                orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=conv), 4)
    if mech in ("h2o2_n16", "h2o2_n32"):      # ng = 16 / 32: the energy instance is one width up from the isothermal one
        d = _h2o2_with_inerts(tmp_path, int(mech[-2:]))
        return (pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=conv),
                orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=conv), 4 if mech[-2:] == "16" else 16)
    f = {"h2o2": "h2o2.dat", "gri": "grimech.dat"}[mech]
    return (pkg.Mechanism.from_files(LIB, gas_mech=f, conv=conv), orc.Mech(os.path.join(LIB, f), TH, None, conv=conv),
            4 if mech == "h2o2" else 16)


@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
@pytest.mark.parametrize("mech", ["h2o2", "s24", "gri", "h2o2_n16", "h2o2_n32"])
def test_energy_rhs_against_the_oracle(pkg, orc, gpu, tmp_path, mech, conv):
    """br_debug_energy_eval (the energy instance's own device functions, launch shape, LDS block and slot,
    constants rebuilt in the live slot) against oracle.rhs at the clamped T and dT/dt from thermo_e_cv, on
    k_integrate<16, 32, 56>'s energy instances (H2/O2, a 24-species GRI subset, GRI; and H2/O2 with inert species
    up to ng = 16 and 32, where ng + 1 selects the next width, not the isothermal instance's). N = 4 x the widest
    workgroup + 3: two workgroups, every wave takes at least a second reactor in the slot of its first.
    Temperatures in both NASA ranges, exactly at a Tmid (1000 K and the mechanism's largest), below 200 K and above 6000 K (clamped), with and
    without rate multipliers. Species rows to 1e-11 of M_k sum_r |nu_kr q_r| (the RHS bar of test_rates_parity's
    scale), dT/dt to 1e-11 of sum_k |e_k w_k| / sum_k c_k cv_k."""
    pm, om, maxrpb = _eval_case(pkg, orc, tmp_path, mech, conv)
    assert pm.ns == 0 and {"h2o2": pm.ng + 1 <= 16, "s24": 17 <= pm.ng + 1 <= 32, "gri": 33 <= pm.ng + 1 <= 56,
                           "h2o2_n16": pm.ng == 16, "h2o2_n32": pm.ng == 32}[mech]
    eng = pkg.Engine(pm)
    N = 4 * maxrpb + 3
    _, p, x, _ = _states(pm, N, 21)
    rng = np.random.default_rng(22)
    T = rng.uniform(300.0, 3200.0, N)
    T[:4] = [1000.0, 150.0, 6500.0, pm.nasa[:, 0].max()]        # (GRI: three species have their Tmid above 1000 K)
    assert np.any(pm.nasa[:, 0] == 1000.0) and (T < 1000.0).sum() > 3 and (T > 1500.0).sum() > 3
    Tc = pm.clamp_T(T)
    U = np.stack([pm.initial_state(Tc[i], p[i], x[i]) for i in range(N)])
    mult = rng.uniform(0.5, 2.0, (3, pm.nrg))
    mult[1, 0] = 0.0
    rows = (np.arange(N) % 3).astype(np.int32)
    worst = [0.0, 0.0]
    for m in (None, mult):
        du = eng.energy_eval(T, U) if m is None else eng.energy_eval(T, U, rate_mult=m, rate_mult_row=rows)
        assert du.shape == (N, pm.ng + 1)
        for i in range(N):
            for r in range(pm.nrg):
                v = 1.0 if m is None else m[rows[i], r]
                om.set_rxn_mult(r, v, v)
            do = om.rhs(float(Tc[i]), 1.0, U[i])[0]
            c = U[i] / pm.molwt
            qg, qs = om.rop(float(Tc[i]), R_GAS * Tc[i] * c.sum(), c / c.sum())
            sc = _scale(pm, qg, qs) * pm.molwt
            e, cv = pm.thermo_e_cv(T[i])
            w = do / pm.molwt
            Td = pm.energy_rhs(do, U[i], T[i])
            sT = np.sum(np.abs(e * w)) / np.sum(c * cv)
            worst[0] = max(worst[0], float(np.max(np.abs(du[i, :-1] - do) / (sc + 1e-300))))
            worst[1] = max(worst[1], abs(du[i, -1] - Td) / sT)
            assert np.all(np.abs(du[i, :-1] - do) <= 1e-11 * sc + 1e-300), (mech, conv, m is not None, i)
            assert abs(du[i, -1] - Td) <= 1e-11 * sT, (mech, conv, m is not None, i, du[i, -1], Td)
    for r in range(pm.nrg):
        om.set_rxn_mult(r, 1.0, 1.0)
    print(f"\n  {mech} conv {conv}: worst species row {worst[0] / 1e-11:.3g}, worst dT/dt {worst[1] / 1e-11:.3g} (units of 1e-11)")
    eng.close()


# --------------------------------------------------------------------------------- 2. trajectories
@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
@pytest.mark.parametrize("name", list(ec.REGIMES))
def test_trajectory_against_the_cpu_statement(pkg, orc, gpu, name, conv):
    """Default tolerances: the GPU's yout and T_out at 28 of the host run's own accepted steps and at tf against
    the host run's states there, per window of t / t_ign (tests/parity_bands.py). The bound of a window is
    2 x the CPU statement's own spread over 6 re-runs from y0 (1 + 1e-15 N(0, 1)), floor 1e-6 band, computed
    here on the host (energy_cases.host_spread; the values are in DESIGN.md). t_ign agrees to
    max(ign_dt of either run, 2 x that spread in t_ign), the step counts to 35 %, nfe_dq == nje (ng + 1)."""
    pm, om, y0, tf = ec.mechs(pkg, orc, name, conv)
    base = ec.host_run(pkg, orc, name, conv)
    spread, dt_spread = ec.host_spread(pkg, orc, name, conv)
    bound = np.maximum(2.0 * spread, 1e-6)
    pk = ec.picks(base)
    tq = base["t"][pk]
    eng = pkg.Engine(pm)
    U, st = eng.integrate([y0[-1]], [1.0], y0[None, :-1], [tf], tout=tq, energy="adiabatic")
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * (pm.ng + 1) and st["nje"][0] > 0
    Yg = np.concatenate([st["yout"][0], st["T_out"][0][:, None]], axis=1)
    e = ec.window_errors(Yg, base["Y"][pk], base["t_ign"], tq)
    e = np.maximum(e, ec.window_errors(np.append(U[0], st["T_end"][0]), base["y"], base["t_ign"], [tf]))
    d_ign = abs(st["t_ign"][0] - base["t_ign"])
    b_ign = max(st["ign_dt"][0], base["ign_dt"], 2.0 * dt_spread)
    print(f"\n  {name} conv {conv}: bands pre / front / post {e[0]:.3g} / {e[1]:.3g} / {e[2]:.3g}, host spread "
          f"{spread[0]:.3g} / {spread[1]:.3g} / {spread[2]:.3g}; t_ign {st['t_ign'][0]:.6g} vs {base['t_ign']:.6g} "
          f"(bound {b_ign:.3g}, host spread {dt_spread:.3g}); T_end {st['T_end'][0]:.2f} vs {base['y'][-1]:.2f}; "
          f"steps {int(st['nsteps'][0])} vs {int(base['stats'][0])}")
    assert np.all(e <= bound), (name, conv, e, bound)
    assert d_ign <= b_ign, (name, conv, d_ign, b_ign)
    assert abs(st["nsteps"][0] - base["stats"][0]) <= 0.35 * base["stats"][0]
    assert _same(st["T_out"][0][-1], st["T_end"][0]) or tq[-1] != tf
    eng.close()


# --------------------------------------------------------------------------------- 3. / 4. converged, conservation
@pytest.mark.parametrize("name", list(ec.REGIMES))
def test_converged_against_radau_and_conservation(pkg, orc, gpu, name):
    """rtol 1e-10 / atol 1e-16, conv = 0, against SciPy's Radau on the CPU statement's f: the end state and T_end
    to 1e-6 relative (floor 1e-14). On the same run, E = internal_energy(yout, T_out) at 28 outputs and at the
    end stays within 4 x the host run's own drift at these tolerances (floor 1e-12 relative: the margin covers
    another step sequence and the device's rounding), and sum_k u_k is constant to 1e-12."""
    pm, om, y0, tf = ec.mechs(pkg, orc, name, 0)
    ref = ec.radau_end(pkg, orc, name)
    host = ec.host_run(pkg, orc, name, 0, rtol=1e-10, atol=1e-16)
    tq = host["t"][ec.picks(host)]
    eng = pkg.Engine(pm)
    U, st = eng.integrate([y0[-1]], [1.0], y0[None, :-1], [tf], rtol=1e-10, atol=1e-16, tout=tq, energy="adiabatic")
    assert st["status"][0] == 0
    e = close_states(np.append(U[0], st["T_end"][0]), ref, rtol=1e-6, floor=1e-14)
    E0 = pm.internal_energy(y0[:-1], y0[-1])
    E = np.append(pm.internal_energy(st["yout"][0], st["T_out"][0]), pm.internal_energy(U[0], st["T_end"][0]))
    drift = float(np.max(np.abs(E / E0 - 1.0)))
    drift_host = float(np.max(np.abs(host["E"] / host["E"][0] - 1.0)))
    rho = np.append(st["yout"][0].sum(axis=1), U[0].sum())
    dm = float(np.max(np.abs(rho / y0[:-1].sum() - 1.0)))
    print(f"\n  {name}: converged error {e:.3g} of the 1e-6 bar, T_end {st['T_end'][0]:.2f} K; E drift {drift:.3g} "
          f"(host {drift_host:.3g}), mass drift {dm:.3g}")
    assert e <= 1.0, (name, e)
    assert drift <= max(4.0 * drift_host, 1e-12), (name, drift, drift_host)
    assert dm <= 1e-12, (name, dm)
    eng.close()


@pytest.mark.parametrize("n", [16, 32])
def test_converged_at_the_width_boundaries(pkg, orc, gpu, tmp_path, n):
    """ng = 16 and 32: the energy instance is k_integrate<32> / <56> (from ng + 1) on a mechanism whose isothermal
    instance is <16> / <32>, with its own LDS block and launch shape. H2/O2 with inert species at zero
    concentration is the same ODE as the nine-species regime: at rtol 1e-10 / atol 1e-16 the shared species and
    T_end agree with its Radau reference to 1e-6 (floor 1e-14), and the inerts stay 0 to that floor (their du is
    exactly 0, but they are third bodies: their Jacobian columns are not empty, the LU may pivot the T row above an
    inert's unit row, and the solve then returns a rounding-sized correction, 1e-27 here, instead of 0)."""
    pm9, _, y9, tf = ec.mechs(pkg, orc, "h2o2", 0)
    ref = ec.radau_end(pkg, orc, "h2o2")
    d = _h2o2_with_inerts(tmp_path, n)
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=0)
    assert pm.ng == n and pm.gas_species[:9] == pm9.gas_species
    r = ec.REGIMES["h2o2"]
    u0 = pm.initial_state(r["T0"], r["p"], pm.mole_fractions(r["x"]))
    assert np.array_equal(u0[:9], y9[:-1]) and not u0[9:].any()
    eng = pkg.Engine(pm)
    U, st = eng.integrate([r["T0"]], [1.0], u0[None, :], [tf], rtol=1e-10, atol=1e-16, energy="adiabatic")
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * (n + 1) and np.all(np.abs(U[0, 9:]) <= 1e-14)
    e = close_states(np.append(U[0, :9], st["T_end"][0]), ref, rtol=1e-6, floor=1e-14)
    print(f"\n  ng = {n}: converged error {e:.3g} of the 1e-6 bar, T_end {st['T_end'][0]:.2f} K")
    assert e <= 1.0, (n, e)
    eng.close()


# --------------------------------------------------------------------------------- 5. bitwise identities
def test_bitwise_identities(pkg, orc, gpu):
    """Five different reactors integrated together equal the same five one at a time; a run with tout equals the
    run without; multipliers all 1.0 equal no multipliers: in U, T_end and every counter, bit for bit."""
    pm, T, Asv, U0, tf = _five(pkg, orc)
    eng = pkg.Engine(pm)
    U, st = eng.integrate(T, Asv, U0, tf, energy="adiabatic")
    assert np.all(st["status"] == 0) and np.ptp(st["T_end"]) > 10.0 and np.all(st["T_end"] > T + 500.0)
    for i in range(5):
        Ui, si = eng.integrate(T[i:i + 1], Asv[i:i + 1], U0[i:i + 1], tf[i:i + 1], energy="adiabatic")
        assert _same(Ui[0], U[i]) and _same(si["T_end"][0], st["T_end"][i]), i
        for k in COUNTERS + TIMES:
            assert _same(si[k][0], st[k][i]), (i, k)
    variants = {"tout": dict(tout=np.array([1e-6, 5e-5, 2e-4, 1e-3])), "ones": dict(rate_mult=np.ones((1, eng.nr)),
                                                                                      rate_mult_row=np.zeros(5, np.int32))}
    for what, kw in variants.items():
        Uv, sv = eng.integrate(T, Asv, U0, tf, energy="adiabatic", **kw)
        assert _same(Uv, U) and _same(sv["T_end"], st["T_end"]), what
        for k in COUNTERS + TIMES:
            assert _same(sv[k], st[k]), (what, k)
        if what == "tout":                      # outputs: u0 / T0 before the first step, the end state at tf
            assert _same(sv["T_out"][:, -1], st["T_end"]) and _same(sv["yout"][:, -1], U)
            assert np.all(np.diff(sv["T_out"], axis=1) >= -1e-6) and np.all(np.abs(sv["T_out"][:, 0] - T) < 1.0)
    eng.close()


# --------------------------------------------------------------------------------- 6. plumbing
def test_multi_phase_and_isothermal_after(pkg, orc, gpu):
    """br_integrate_multi (two handles, slices of 3 and 2) equals the single call, T_end and T_out sliced with
    the ensemble; integrate_phase puts T_out at tau x t_ign; an isothermal run on the handle after the energy
    runs is bitwise the one before them."""
    pm, T, Asv, U0, tf = _five(pkg, orc)
    eng, e2 = pkg.Engine(pm), pkg.Engine(pm)
    Ui0, si0 = eng.integrate(T, Asv, U0, tf, dq_jacobian=True)
    tout = np.array([2e-5, 1e-4, 1e-3])
    U, st = eng.integrate(T, Asv, U0, tf, tout=tout, energy="adiabatic")
    Um, sm = pkg.integrate_multi([eng, e2], T, Asv, U0, tf, tout=tout, energy="adiabatic")
    assert np.all(st["status"] == 0) and _same(Um, U)
    for k in COUNTERS + TIMES + ("T_end", "T_out", "yout"):
        assert _same(sm[k], st[k]), k
    tau = np.array([0.5, 1.0, 2.0])
    Up, sp = eng.integrate_phase(T, Asv, U0, tf, tau, energy="adiabatic")
    assert _same(Up, U) and _same(sp["t_ign"], st["t_ign"]) and _same(sp["T_end"], st["T_end"])
    assert _same(sp["tout"], pkg.phase_grid(st["t_ign"], tau, tf)) and np.all(np.isfinite(sp["tout"]))
    U2, s2 = eng.integrate(T, Asv, U0, tf, tout=sp["tout"], energy="adiabatic")
    assert _same(sp["T_out"], s2["T_out"]) and _same(sp["yout"], s2["yout"])
    assert np.all(sp["T_out"][:, 0] < sp["T_out"][:, 1]) and np.all(sp["T_out"][:, 1] < sp["T_out"][:, 2])   # T rises through the front
    Ui1, si1 = eng.integrate(T, Asv, U0, tf, dq_jacobian=True)
    assert _same(Ui1, Ui0)
    for k in COUNTERS + TIMES:
        assert _same(si1[k], si0[k]), k
    assert not _same(U, Ui0)                                            # (the energy equation does change the run)
    eng.close()
    e2.close()


def test_sensitivity_is_the_quotient_of_explicit_runs(pkg, orc, gpu):
    """sensitivity(energy="adiabatic") on 2 H2/O2 reactors x 3 reactions equals the central difference formed
    from explicit rate_mult runs with the same factor (the expanded reactors are those runs), at the bounds of
    test_sensitivity_equals_explicit_runs: S_u is one subtraction and one division of the same numbers, 1e-14
    relative; S_tign differs by the device's log, 1e-14 (|ln t+| + |ln t-|) / (2 ln f). It differs from the
    isothermal sensitivity."""
    pm, T, Asv, U0, tf = _five(pkg, orc)
    T, Asv, U0, tf = T[:2], Asv[:2], U0[:2], tf[:2]
    eng = pkg.Engine(pm)
    rx, f = np.array([0, 3, 8], np.int32), 1.5
    out = eng.sensitivity(T, Asv, U0, tf, factor=f, reactions=rx, states=True, energy="adiabatic")
    iso = eng.sensitivity(T, Asv, U0, tf, factor=f, reactions=rx, states=True, dq_jacobian=True)
    assert out["nbad"] == 0 and not _same(out["S_tign"], iso["S_tign"]) and np.abs(out["S_tign"]).max() > 0.05
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


def test_unsupported_cases(pkg, gpu):
    """BR_ERR_UNSUPPORTED, each with its message: a mechanism with surface species, a traced run, and (when one
    can be had) ng + 1 > 56 -- none can: the widest gas mechanism in the library, GRI-Mech 3.0, has 53 species."""
    sm = pkg.Mechanism.from_files(LIB, surface_mech="ch4ni.xml", gasphase=SURF_GAS)
    eng = pkg.Engine(sm)
    u0 = sm.initial_state(1000.0, 1e5, sm.mole_fractions({"CH4": 0.5, "N2": 0.5}))
    with pytest.raises(RuntimeError, match=r"-30: br_opts.energy: mechanisms with surface species"):
        eng.integrate([1000.0], [1.0], u0[None, :], [1e-3], energy="adiabatic")
    with pytest.raises(RuntimeError, match=r"-30: br_opts.energy: mechanisms with surface species"):
        eng.energy_eval([1000.0], u0[None, :sm.ng])
    eng.close()
    pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat")
    eng = pkg.Engine(pm)
    u0 = pm.initial_state(1100.0, 1e5, pm.mole_fractions({"H2": 0.3, "O2": 0.2, "N2": 0.5}))
    with pytest.raises(RuntimeError, match=r"-30: br_integrate_traced does not take br_opts.energy"):
        eng.integrate([1100.0], [1.0], u0[None, :], [1e-3], trace_cap=100, energy="adiabatic")
    eng.close()
    assert pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat").ng + 1 <= 56
