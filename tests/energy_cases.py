"""Shared cases of the adiabatic constant-volume tests (br_opts.energy; test infrastructure for
test_energy_host.py and test_energy_gpu.py). The CPU statement of an energy run is br_integrate_host with
f(t, [u, T]) = [oracle.rhs(Tc, 1, u), dT/dt from Mechanism.thermo_e_cv]: the same CVODE restatement with a DQ
Jacobian over ng + 1 columns. SciPy's Radau on the same f is the converged reference. Everything here runs on
the CPU; results are computed once per process and shared (callers must not modify them).

Regimes (no regime starts at a species' Tmid, 1000 K: the NASA fits jump there, which shows as a 2e-7 step in E):
  h2o2  {H2 .3, O2 .2, N2 .5}, 1e5 Pa, T0 = 1100 K, tf = 1e-3 s: ignites near 5.8e-5 s
  gri   {CH4 .1, O2 .2, N2 .7}, 1e5 Pa, T0 = 1500 K, tf = 5e-3 s: ignites near 1.06e-3 s (conv = 0)
"""
import os

import numpy as np

from conftest import LIB
from parity_bands import band_errors

TH = os.path.join(LIB, "therm.dat")
REGIMES = {
    "h2o2": dict(mech="h2o2.dat", x={"H2": 0.3, "O2": 0.2, "N2": 0.5}, p=1e5, T0=1100.0, tf=1e-3),
    "gri": dict(mech="grimech.dat", x={"CH4": 0.1, "O2": 0.2, "N2": 0.7}, p=1e5, T0=1500.0, tf=5e-3),
}
NPICK = 28          # accepted steps of the host run at which trajectories are compared
NRERUN = 6          # re-runs of the CPU statement from u0 (1 + 1e-15 N(0, 1)) for its own spread
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def mechs(pkg, orc, name, conv):
    """(product mechanism, oracle mechanism, y0 = [u0, T0], tf) of a regime"""
    def make():
        r = REGIMES[name]
        pm = pkg.Mechanism.from_files(LIB, gas_mech=r["mech"], conv=conv)
        om = orc.Mech(os.path.join(LIB, r["mech"]), TH, None, conv=conv)
        u0 = pm.initial_state(r["T0"], r["p"], pm.mole_fractions(r["x"]))
        return pm, om, np.append(u0, r["T0"]), r["tf"]
    return _memo(("mechs", name, conv), make)


def rhs_fn(pm, om):
    """f(t, [u, T]) of the model in include/brhip.h: the species RHS at the clamped T, dT/dt from its own du"""
    def f(_t, y):
        u, T = y[:-1], y[-1]
        du = om.rhs(float(pm.clamp_T(T)), 1.0, u)[0]
        return np.append(du, pm.energy_rhs(du, u, T))
    return f


def radau_end(pkg, orc, name):
    """[u, T] at tf from SciPy's Radau at rtol 1e-10 / atol 1e-16, conv = 0"""
    def make():
        from scipy.integrate import solve_ivp
        pm, om, y0, tf = mechs(pkg, orc, name, 0)
        sol = solve_ivp(rhs_fn(pm, om), (0.0, tf), y0, method="Radau", rtol=1e-10, atol=1e-16)
        assert sol.status == 0, sol.message
        return sol.y[:, -1].copy()
    return _memo(("radau", name), make)


def ignition_from_steps(pm, t, Y):
    """(t_ign, ign_dt) as br_stats has them, from accepted steps (t[0] = 0): the midpoint and width of the step
    with the largest dX_OH/dt"""
    k = pm.gas_species.index("OH")
    c = Y[:, :pm.ng] / pm.molwt
    x = c[:, k] / c.sum(axis=1)
    rate = np.diff(x) / np.diff(t)
    i = int(np.argmax(rate))
    return 0.5 * (t[i] + t[i + 1]), t[i + 1] - t[i]


def host_run(pkg, orc, name, conv, rtol=1e-6, atol=1e-10, seed=None):
    """The CPU statement of an energy run: dict with the accepted steps t [m], Y [m, ng + 1] (row 0: t = 0, the
    last row: tf), the end state y, stats, t_ign / ign_dt, and E = internal_energy at every step. seed: start
    from y0 (1 + 1e-15 N(0, 1)) instead."""
    def make():
        pm, om, y0, tf = mechs(pkg, orc, name, conv)
        if seed is not None:
            y0 = y0 * (1.0 + 1e-15 * np.random.default_rng(seed).standard_normal(y0.size))
        rows = []
        status, y, st = pkg._lib.integrate_host(rhs_fn(pm, om), y0, tf, rtol=rtol, atol=atol,
                                                on_step=lambda t, u: rows.append((t, u)))
        assert status == 0, (name, conv, status)
        t = np.array([r[0] for r in rows])
        Y = np.array([r[1] for r in rows])
        if t[-1] - t[-2] <= 1e-12 * tf:          # (the tf row repeats the last accepted step, which lands on tf)
            t, Y = np.delete(t, -2), np.delete(Y, -2, axis=0)
        tign, dt = ignition_from_steps(pm, t, Y)
        return dict(t=t, Y=Y, y=y, stats=st, t_ign=tign, ign_dt=dt, E=pm.internal_energy(Y[:, :-1], Y[:, -1]))
    return _memo(("host", name, conv, rtol, atol, seed), make)


def picks(run):
    """indices of NPICK accepted steps of a host run (never row 0), the last one tf"""
    return np.unique(np.linspace(1, len(run["t"]) - 1, NPICK).astype(int))


def _hermite(f, t, Y, tq):
    """cubic Hermite interpolant of the steps (t, Y) with slopes f(t_i, Y_i), at the times tq"""
    out = np.empty((len(tq), Y.shape[1]))
    for j, x in enumerate(tq):
        i = min(max(int(np.searchsorted(t, x, side="right")) - 1, 0), len(t) - 2)
        h = t[i + 1] - t[i]
        s = (x - t[i]) / h
        f0, f1 = f(t[i], Y[i]), f(t[i + 1], Y[i + 1])
        out[j] = ((2 * s ** 3 - 3 * s ** 2 + 1) * Y[i] + (s ** 3 - 2 * s ** 2 + s) * h * f0
                  + (-2 * s ** 3 + 3 * s ** 2) * Y[i + 1] + (s ** 3 - s ** 2) * h * f1)
    return out


def window_errors(Yg, Yo, t_ign, tout):
    """band errors per ignition window (tests/parity_bands.py), T as one more column of the state"""
    return np.array(band_errors(np.atleast_2d(Yg), np.atleast_2d(Yo), t_ign, np.atleast_1d(np.asarray(tout, float))))


def host_spread(pkg, orc, name, conv):
    """The CPU statement's own spread at default tolerances (the method of DESIGN.md section 1): NRERUN re-runs
    from y0 (1 + 1e-15 N(0, 1)) against the unperturbed run, at NPICK of its accepted steps and at tf, in bands
    per ignition window; and the largest shift of t_ign. A re-run takes other steps, so its states at the
    unperturbed run's step times come from the cubic Hermite interpolant of its own accepted steps (error
    O(h^4), the order of a dense output's own; at tf the states are compared directly).
    Returns (spread [3], spread of t_ign)."""
    def make():
        pm, om, _, tf = mechs(pkg, orc, name, conv)
        f = rhs_fn(pm, om)
        base = host_run(pkg, orc, name, conv)
        pk = picks(base)
        tq = base["t"][pk]
        e, dt = np.zeros(3), 0.0
        for seed in range(NRERUN):
            r = host_run(pkg, orc, name, conv, seed=100 + seed)
            Yr = _hermite(f, r["t"], r["Y"], tq[:-1])
            e = np.maximum(e, window_errors(Yr, base["Y"][pk[:-1]], base["t_ign"], tq[:-1]))
            e = np.maximum(e, window_errors(r["y"], base["y"], base["t_ign"], [tf]))
            dt = max(dt, abs(r["t_ign"] - base["t_ign"]))
        return e, dt
    return _memo(("spread", name, conv), make)
