"""Prescribed temperature programmes T(t) in the wavefront engine (br_opts.ntprog), on the GPU: the device
evaluator on its own, a constant programme against the isothermal run (bit for bit: the refresh rule and
its "never refreshes" path), the time-scaling identity (every RHS sees the time the controller means),
trajectories against the host CVODE restatement f(t, u) = oracle.rhs(T(t), Asv, u), converged runs against
SciPy's Radau on the same RHS, and the plumbing of the other entry points."""
import os

import numpy as np
import pytest

from conftest import LIB
from parity_bands import BOUNDS, band_errors
from test_gpu_parity import SURF_GAS, TH, close_states

pytestmark = pytest.mark.gpu

R_GAS = 8.31446261815324
COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "nfe_dq")
TIMES = ("t_end", "t_ign", "ign_dt")
# which -> (case, N, programme kernel's isothermal twin, tf)
WAVE = {"wave16": ("h2o2", 6, "k_integrate<16>", 2e-3), "wave32": ("surf", 9, "k_integrate<32>", 1.0),
        "wave56": ("gri", 5, "k_integrate<56>", 1e-2), "wave72": ("gas_surf", 3, "k_integrate<72>", 1e-2)}
FILES = {"h2o2": dict(gas_mech="h2o2.dat"), "gri": dict(gas_mech="grimech.dat"),
         "surf": dict(surface_mech="ch4ni.xml", gasphase=SURF_GAS),
         "gas_surf": dict(gas_mech="grimech.dat", surface_mech="ch4ni.xml")}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _case(pkg, monkeypatch, which):
    """(mechanism, engine, T, Asv, U0, tf, N) of a WAVE entry on the wavefront engine (the isothermal run the
    programme run is compared with must be that engine's: BRHIP_ENGINE = wave, as the existing tests do)"""
    from batchreactor_amd import ensemble
    case, N, kernel, tf = WAVE[which]
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    pm = pkg.Mechanism.from_files(LIB, **FILES[case])
    T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    eng = pkg.Engine(pm)
    assert eng.kernel_name == kernel, eng.kernel_name
    return pm, eng, T, Asv, U0, np.full(N, tf), N


def _oracle(orc, case):
    f = FILES[case]
    gm, sm = f.get("gas_mech"), f.get("surface_mech")
    return orc.Mech(os.path.join(LIB, gm) if gm else None, TH, os.path.join(LIB, sm) if sm else None,
                    gas_species=None if gm else SURF_GAS, conv=orc.CONV_REFERENCE)


# --------------------------------------------------------------------------------- 1. the evaluator
def _eval_dev(pkg, kt, kT, rows, t):
    L = pkg._lib
    kt, kT = np.ascontiguousarray(kt, np.float64), np.ascontiguousarray(kT, np.float64)
    t = np.ascontiguousarray(t, np.float64)
    N, nt = t.shape
    out = np.full((N, nt), -1.0)
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    rc = L.lib().br_debug_tprog_eval(N, kt.shape[1], L.dptr(kt), L.dptr(kT), kt.shape[0], L.iptr(r), nt, L.dptr(t),
                                     L.dptr(out))
    assert rc == 0, L.lib().br_last_error()
    return out


def test_device_evaluator_against_numpy(pkg, gpu):
    """br_debug_tprog_eval (the integrator's evaluator) against the header's formula in numpy, to 1e-14
    relative (the three operations may be contracted on the device): shared and per-reactor rows, ragged
    rows, a one-knot row, a jump, times exactly on knots, past the end, and in descending order (the scan
    from the cached segment goes both ways). 70 reactors: more than one block of the check kernel."""
    rng = np.random.default_rng(5)
    nrows, nk, N = 7, 6, 70
    kt = np.cumsum(rng.uniform(0.05, 2.0, (nrows, nk)), axis=1)
    kt[:, 0] = 0.0
    kT = rng.uniform(300.0, 1500.0, (nrows, nk))
    kt[1, 3:] = np.nan                                   # ragged: three knots
    kt[2, 1:] = np.nan                                   # one knot: constant
    kt[3, 3] = kt[3, 2]                                  # a jump
    kT[1, 4] = np.nan                                    # (under padding: not read)
    tmax = np.nanmax(kt) * 1.3
    rows = rng.integers(0, nrows, N)
    rows[:nrows] = np.arange(nrows)
    base = np.concatenate([rng.uniform(0.0, tmax, 40), [0.0, tmax, 1e6]])
    for order in ("random", "ascending", "descending"):
        t = np.empty((N, base.size + nk))
        for i in range(N):
            knots = np.where(np.isnan(kt[rows[i]]), 0.0, kt[rows[i]])       # exactly on the row's own knots
            ti = np.concatenate([base, knots])
            t[i] = ti if order == "random" else np.sort(ti) if order == "ascending" else np.sort(ti)[::-1]
        want = np.array([pkg.tprog.evaluate(kt[rows[i]], kT[rows[i]], t[i]) for i in range(N)])
        got = _eval_dev(pkg, kt, kT, rows, t)
        assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), (order, np.abs(got / want - 1).max())
        for i in range(N):                                                    # on a knot: the knot's T itself, exactly
            on = np.isin(t[i], kt[rows[i]][~np.isnan(kt[rows[i]])])
            assert on.sum() >= 2 and np.array_equal(got[i][on], want[i][on]), (order, i)
    # per-reactor rows (tprog_row NULL, nrows == N)
    t7 = np.tile(base, (nrows, 1))
    got = _eval_dev(pkg, kt, kT, None, t7)
    want = np.array([pkg.tprog.evaluate(kt[i], kT[i], t7[i]) for i in range(nrows)])
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want))
    assert np.all(got[2] == kT[2, 0]) and np.all(got[:, -1] == [kT[i, np.count_nonzero(~np.isnan(kt[i])) - 1] for i in range(nrows)])


# --------------------------------------------------------------------------------- 2. constant programme
@pytest.mark.parametrize("which", list(WAVE))
def test_constant_programme_is_the_isothermal_run(pkg, gpu, monkeypatch, which):
    """T(t) = T_i for every t -- two knots, and a ragged row padded with NaN -- gives the states, the dense
    outputs and every solver counter of the plain wavefront-engine run, bit for bit, with the analytic and
    the DQ Jacobian, with rate multipliers on (every second reactor's reactions at 1.5) and off, and with
    T = None (the argument is not read). The constants are built once at T(0) and never refreshed."""
    pm, eng, T, Asv, U0, tf, N = _case(pkg, monkeypatch, which)
    tout = np.array([1e-6, 1e-4, 0.5, 1.0]) * tf[0]
    two = (np.stack([np.zeros(N), tf / 3], axis=1), np.stack([T, T], axis=1))
    ragged = (np.stack([np.zeros(N), 0.7 * tf, np.full(N, np.nan), np.full(N, np.nan)], axis=1),
              np.stack([T, T, np.full(N, np.nan), np.full(N, -1.0)], axis=1))
    mult = np.ones((N, eng.nr))
    mult[1::2] = 1.5
    for dq in (False, True):
        for m in (None, mult) if which in ("wave32", "wave56") or not dq else (None,):
            U, st = eng.integrate(T, Asv, U0, tf, tout=tout, dq_jacobian=dq, rate_mult=m)
            assert np.all(st["nsteps"] > 0) and np.all(st["status"] == 0)
            for name, prog, Targ in (("two knots", two, T), ("ragged", ragged, None)):
                Up, sp = eng.integrate(Targ, Asv, U0, tf, tout=tout, dq_jacobian=dq, rate_mult=m, tprog=prog)
                what = (which, dq, m is not None, name)
                assert _same(Up, U), what
                assert _same(sp["yout"], st["yout"]), what
                for k in COUNTERS + TIMES + ("ign_rate",):
                    assert _same(sp[k], st[k]), what + (k,)


# --------------------------------------------------------------------------------- 3. time-scaling identity
def _kinked(T, tf, N):
    """per-reactor programmes with a kink inside (0, tf): up 60 K by tf / 4, down 20 K by 0.6 tf, held"""
    kt = np.stack([np.zeros(N), tf / 4, 0.6 * tf], axis=1)
    kT = np.stack([T, T + 60.0, T + 40.0], axis=1)
    return kt, kT


@pytest.mark.parametrize("which", ["wave16", "wave32", "wave56"])
def test_time_scaling_identity(pkg, gpu, monkeypatch, which):
    """Knots (t_j / 2, T_j), every rate multiplier 2 and tf / 2 reproduce the (t_j, T_j) run: the same states
    and counters, exactly half the times (every quantity scales by a power of two, and so does the
    programme's argument). A right-hand side evaluated at another time than the controller's -- tn instead
    of tn + hg in the initial-step estimate, a stale tn after a rejected step -- breaks it. Both Jacobians."""
    pm, eng, T, Asv, U0, tf, N = _case(pkg, monkeypatch, which)
    kt, kT = _kinked(T, tf, N)
    two = np.full((1, eng.nr), 2.0)
    rows = np.zeros(N, np.int32)
    U0_, _ = eng.integrate(T, Asv, U0, tf)
    for dq in (False, True):
        U, st = eng.integrate(None, Asv, U0, tf, dq_jacobian=dq, tprog=(kt, kT))
        assert np.all(st["status"] == 0) and not _same(U, U0_)           # (the programme does change the run)
        Um, sm = eng.integrate(None, Asv, U0, tf / 2, dq_jacobian=dq, tprog=(kt / 2, kT), rate_mult=two, rate_mult_row=rows)
        for k in COUNTERS:
            assert _same(sm[k], st[k]), (which, dq, k)
        assert _same(Um, U), (which, dq)
        for k in TIMES:
            assert _same(sm[k], st[k] / 2), (which, dq, k)
        assert _same(sm["ign_rate"], st["ign_rate"] * 2), (which, dq)


# --------------------------------------------------------------------------------- 4. / 5. trajectories
def _regime(pkg, name):
    """(case, mechanism, Asv, u0, programme, tf) of the three regimes without a rounding-chaotic front"""
    from batchreactor_amd import ensemble
    TP = pkg.TemperatureProgram
    if name == "surf_tpd":            # a surface ramp from the mechanism's adsorbed layer: 150 K/s for 1 s, then held
        pm = pkg.Mechanism.from_files(LIB, **FILES["surf"])
        T, Asv, U0 = ensemble.make_inputs(pm, "surf", 3, 1)
        return "surf", pm, Asv[0], U0[0], TP.from_knots([0.0, 1.0, 1.5], [T[0], T[0] + 150.0, T[0] + 150.0]), 1.5
    if name in ("h2o2_ramp", "h2o2_ramp700"):   # H2/O2/N2 heated T0 -> T0 + 80 K in 0.6 ms, then cooled: no ignition before 1 ms
        T0 = 800.0 if name == "h2o2_ramp" else 700.0
        pm = pkg.Mechanism.from_files(LIB, **FILES["h2o2"])
        x = pm.mole_fractions({"H2": 0.3, "O2": 0.2, "N2": 0.5})
        return "h2o2", pm, 1.0, pm.initial_state(T0, 1e5, x), TP.from_knots([0.0, 6e-4, 1e-3], [T0, T0 + 80.0, T0 + 50.0]), 1e-3
    pm = pkg.Mechanism.from_files(LIB, **FILES["gri"])   # GRI, CH4/O2/N2 at 950 -> 1050 K: below ignition at 1 ms
    x = pm.mole_fractions({"CH4": 0.1, "O2": 0.2, "N2": 0.7})
    return "gri", pm, 1.0, pm.initial_state(950.0, 1e5, x), TP.from_knots([0.0, 5e-4, 1e-3], [950.0, 1050.0, 1050.0]), 1e-3


@pytest.mark.parametrize("name", ["surf_tpd", "h2o2_ramp", "gri_ramp"])
def test_trajectory_against_the_host_cvode_restatement(pkg, orc, gpu, monkeypatch, name):
    """The CPU statement of a programme run is br_integrate_host with f(t, u) = oracle.rhs(T(t), Asv, u): the
    same CVODE restatement with the DQ Jacobian. The GPU run (dq_jacobian) is compared with it at the host
    run's own accepted steps (its states there against the GPU's dense output at the same times) and at tf,
    within the pre-ignition band bound of the mechanism's DQ runs (tests/parity_bands.py: the programme
    adds no source of rounding), and in its step count as the isothermal DQ parity tests do (35 %)."""
    case, pm, Asv, u0, prog, tf = _regime(pkg, name)
    om = _oracle(orc, case)
    rows = []
    status, uh, sh = pkg._lib.integrate_host(lambda t, u: om.rhs(prog(t), Asv, u)[0], u0, tf,
                                             on_step=lambda t, u: rows.append((t, u)))
    assert status == 0
    th = np.array([r[0] for r in rows[1:]])                     # accepted steps, the last one tf
    Yh = np.array([r[1] for r in rows[1:]])
    pick = np.unique(np.linspace(0, len(th) - 1, 28).astype(int))
    eng = pkg.Engine(pm)
    U, st = eng.integrate(None, [Asv], u0[None, :], [tf], dq_jacobian=True, tprog=prog, tout=th[pick])
    assert st["status"][0] == 0 and st["nfe_dq"][0] == st["nje"][0] * pm.n
    bound = BOUNDS[(case, True)][0]
    e = band_errors(st["yout"][0], Yh[pick], np.nan, th[pick])[0]
    e_end = band_errors(U, uh[None, :], np.nan, np.array([tf]))[0]
    print(f"\n  {name}: {e:.3g} / {e_end:.3g} bands at the steps / at tf (bound {bound}), steps {int(st['nsteps'][0])} vs {int(sh[0])}")
    assert e <= bound and e_end <= bound, (name, e, e_end, bound)
    assert abs(st["nsteps"][0] - sh[0]) <= 0.35 * sh[0], (st["nsteps"][0], sh[0])


@pytest.mark.parametrize("name", ["h2o2_ramp700", "gri_ramp"])
def test_converged_against_radau(pkg, orc, gpu, name):
    """rtol 1e-10 / atol 1e-16 with the analytic Jacobian against SciPy's Radau (rtol 1e-10) on the same
    oracle right-hand side: the end states agree to 1e-6 relative (floor 1e-14), the converged-parity bar
    of test_integrate_parity_tight. The programmes have a kink inside (0, tf); Radau is stopped there.
    The regimes are ones in which CVODE's own truncation error at these tolerances is well inside that bar,
    judged on the CPU alone: br_integrate_host (the same algorithm, DQ Jacobian) against Radau gives 0.33 of
    the bar for the 700 K H2/O2 ramp. The 800 K ramp of the trajectory test is no such regime: its radical
    pool grows by chain branching and amplifies the BDF's truncation error, the CPU restatement is 6.5 bars
    from Radau there (1.3 at 750 K, 3.2 at 780 K; Radau at rtol 1e-10 and 1e-13 agree to 3e-4 of the bar), and
    the GPU run 4.5. SciPy's Radau does not finish the surface ramp in minutes, so it is not among the cases."""
    from scipy.integrate import solve_ivp
    case, pm, Asv, u0, prog, tf = _regime(pkg, name)
    om = _oracle(orc, case)
    y, t0 = np.array(u0), 0.0
    for t1 in list(prog.t[(prog.t > 0) & (prog.t < tf)]) + [tf]:
        y = solve_ivp(lambda t, u: om.rhs(prog(t), Asv, u)[0], (t0, t1), y, method="Radau", rtol=1e-10, atol=1e-16).y[:, -1]
        t0 = t1
    U, st = pkg.Engine(pm).integrate(None, [Asv], u0[None, :], [tf], rtol=1e-10, atol=1e-16, tprog=prog)
    assert st["status"][0] == 0
    e = close_states(U[0], y, rtol=1e-6, floor=1e-14)
    print(f"\n  {name}: converged error {e:.3g} (units of 1e-6 |u| + 1e-14)")
    assert e <= 1.0, (name, e)


# --------------------------------------------------------------------------------- 6. plumbing
def test_multi_phase_and_traced_take_a_programme(pkg, gpu, monkeypatch):
    """br_integrate_multi with a shared row and with per-reactor rows equals the single-device call (N = 7:
    slices of 4 and 3); br_integrate_phase and br_integrate_traced accept a programme; the trace's p_last is
    the pressure diagnosed at T(t) of the row's step (all RHS evaluations of a step are at its tn)."""
    pm, eng, T, Asv, U0, tf, _ = _case(pkg, monkeypatch, "wave16")
    from batchreactor_amd import ensemble
    N = 7
    T, Asv, U0 = ensemble.make_inputs(pm, "h2o2", 0, N)
    tf = np.full(N, 2e-3)
    kt, kT = _kinked(T, tf, N)
    shared = pkg.TemperatureProgram.from_knots([0.0, 5e-4, 1e-3], [1100.0, 1200.0, 1150.0])
    e2 = pkg.Engine(pm)
    for kw in (dict(tprog=(kt, kT)), dict(tprog=shared), dict(tprog=(kt[:3], kT[:3]), tprog_row=np.arange(N) % 3)):
        U1, s1 = eng.integrate(None, Asv, U0, tf, **kw)
        Um, sm = pkg.integrate_multi([eng, e2], None, Asv, U0, tf, **kw)
        assert np.all(s1["status"] == 0) and _same(Um, U1), list(kw)
        for k in COUNTERS + TIMES:
            assert _same(sm[k], s1[k]), (list(kw), k)
    # a bad row is named by its index in the ensemble, not in its slice
    bad = kt.copy()
    bad[5, 2] = 1e-9
    with pytest.raises(RuntimeError, match=r"-10: temperature programme of reactor 5 \(row 5\)"):
        pkg.integrate_multi([eng, e2], None, Asv, U0, tf, tprog=(bad, kT))
    with pytest.raises(RuntimeError, match=r"-30: br_sensitivity"):
        eng.sensitivity(T, Asv, U0, tf, tprog=shared)
    # phase sampling: pass 2 repeats pass 1's steps, so its t_ign is the plain programme run's
    U1, s1 = eng.integrate(None, Asv, U0, tf, tprog=(kt, kT))
    Up, sp = eng.integrate_phase(None, Asv, U0, tf, [0.5, 1.0], tprog=(kt, kT))
    assert _same(Up, U1) and _same(sp["t_ign"], s1["t_ign"]) and np.isfinite(sp["tout"]).any()
    # traced
    cap = 4000
    Ut, stt, tr = eng.integrate(None, Asv[:2], U0[:2], tf[:2], trace_cap=cap, tprog=(kt[:2], kT[:2]))
    assert _same(Ut, U1[:2]) and _same(stt["nsteps"], s1["nsteps"][:2])
    for i in range(2):
        ns = int(stt["nsteps"][i])
        assert 1 < ns < cap
        r = tr[i, 1:ns + 1]
        Tt = pkg.tprog.evaluate(kt[i], kT[i], r[:, 0])
        p_want = R_GAS * Tt * (r[:, 4 + pm.n:4 + pm.n + pm.ng] / pm.molwt).sum(axis=1)
        assert np.all(np.abs(r[:, 3] - p_want) <= 1e-12 * p_want), np.abs(r[:, 3] / p_want - 1).max()
        assert np.ptp(Tt) > 50.0                                         # (the rows do span the ramp)
